"""ctypes binding of include/dpx_align.h (libdpxalign.so).

Every function here goes straight through the C ABI; nothing is computed in Python.  The library is
built in-tree by ``__graft_entry__.build()`` (``make -C dpx_gpu_genomics_project_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np

ALGO_LNW, ALGO_LSW, ALGO_ANW, ALGO_BSW, ALGO_ASW, ALGO_BASW, ALGO_ASG, ALGO_BANW = 0, 1, 2, 3, 4, 5, 6, 7
ALGO_BAXT = 10  # (8 and 9 are unassigned)
ALGO_NAMES = {ALGO_LNW: "LNW", ALGO_LSW: "LSW", ALGO_ANW: "ANW", ALGO_BSW: "BSW", ALGO_ASW: "ASW", ALGO_BASW: "BASW", ALGO_ASG: "ASG",
              ALGO_BANW: "BANW", ALGO_BAXT: "BAXT"}
KEEP_MATRICES, SCORE_ONLY, TIME_FILLS, TUNE_PLACEMENT, KEEP_DIRECTIONS = 0x0, 0x1, 0x2, 0x4, 0x8
KEEP_BAND_DIRECTIONS = 0x10  # BANW / BAXT: 4-bit direction codes per in-band cell, int32 scores (0x8 stays refused on banded algorithms)
KEEP_LOCAL_BAND_DIRECTIONS = 0x40  # BSW / BASW: 4-bit direction codes per in-band cell, int32 scores (0x8 and 0x10 stay refused on them)
TWO_PIECE_GAPS = 0x20  # with KEEP_BAND_DIRECTIONS: a second gap piece (Batch.set_second_gap), 8-bit codes, bands up to 256
LOCAL_TWO_PIECE_GAPS = 0x80  # with KEEP_LOCAL_BAND_DIRECTIONS on BASW: a second gap piece (Batch.set_second_gap), 8-bit codes, bands up to 256
LONG_SCORES = 0x100  # with exactly one of KEEP_BAND_DIRECTIONS / KEEP_LOCAL_BAND_DIRECTIONS: that batch's int32 fill with nothing stored but the results (no pool)
MAT_H, MAT_I, MAT_D = 0, 1, 2
MAT_I2, MAT_D2, MAT_H_PIECE = 3, 4, 5  # Batch.directions on a TWO_PIECE_GAPS batch: piece 2's planes, and the piece of H's gap move
# CIGARs (dpx_batch_cigars_begin / _end): an op is (length << 4) | code with BAM's code numbers
CIGAR_OP_M, CIGAR_OP_I, CIGAR_OP_D, CIGAR_OP_EQ, CIGAR_OP_X = 0, 1, 2, 7, 8
CIGAR_EXTENDED, CIGAR_M = 0x0, 0x1
# difference strings (dpx_batch_diffs_begin / _end): SAM's MD tag, minimap2's short cs tag
DIFF_MD, DIFF_CS = 0x1, 0x2
# BAXT's extension mode (dpx_batch_set_extension / dpx_batch_extensions)
EXT_ZDROPPED, EXT_REACHED_END = 0x1, 0x2
EXT_NO_QUERY_END = -2**31

# every symbol include/dpx_align.h declares (tests check the .so exports all of them)
ABI_VERSION_NEEDED = 3  # include/dpx_align.h DPX_ABI_VERSION: round-3 entry points (dpx_pool_reserve, dpx_batch_last_output_usec) + the pool record in dpx_batch_describe

ABI_SYMBOLS = (
    "dpx_init", "dpx_device_count", "dpx_device_info", "dpx_shutdown", "dpx_pool_reserve", "dpx_text_reserve", "dpx_strerror", "dpx_last_error",
    "dpx_abi_version", "dpx_batch_create", "dpx_batch_create_on", "dpx_pack2", "dpx_batch_create_packed2", "dpx_batch_fill", "dpx_batch_fill_timed", "dpx_batch_last_fill_usec", "dpx_batch_last_output_usec", "dpx_batch_sync",
    "dpx_batch_device_results", "dpx_batch_results", "dpx_batch_matrix", "dpx_batch_traceback",
    "dpx_batch_output_begin", "dpx_batch_output_end", "dpx_batch_output_take", "dpx_text_free",
    "dpx_batch_info", "dpx_batch_describe", "dpx_batch_destroy", "dpx_align_batch", "dpx_prim_eval", "dpx_batch_directions",
    "dpx_batch_cigars_begin", "dpx_batch_cigars_end", "dpx_cigar_text", "dpx_batch_set_extension", "dpx_batch_extensions",
    "dpx_batch_set_substitution", "dpx_batch_set_extension_table", "dpx_batch_set_direction_scoring",
    "dpx_batch_set_second_gap", "dpx_batch_set_reversed", "dpx_batch_set_direction_table",
    "dpx_batch_set_score_table", "dpx_batch_diffs_begin", "dpx_batch_diffs_end", "dpx_batch_set_local_direction_table",
)
# declared entry points a library may lack and still load (an older build): checked when they are called
OPTIONAL_SYMBOLS = ("dpx_batch_directions",)


class DpxError(RuntimeError):
    def __init__(self, status: int, what: str):
        super().__init__(f"{what}: status {status}")
        self.status = status


class SeqPair(C.Structure):
    """== struct seqPair of the reference (c++/parseInput.h:22-29)."""
    _fields_ = [("referenceIdx", C.c_int32), ("referenceSize", C.c_int32), ("queryIdx", C.c_int32),
                ("querySize", C.c_int32)]


class Params(C.Structure):
    _fields_ = [("algo", C.c_int32), ("match", C.c_int32), ("mismatch", C.c_int32), ("gapOpen", C.c_int32),
                ("gapExtend", C.c_int32), ("band", C.c_int32)]


PAIR_DTYPE = np.dtype([("referenceIdx", "<i4"), ("referenceSize", "<i4"), ("queryIdx", "<i4"), ("querySize", "<i4")])
# == struct dpx_alignment (48 bytes): one record per pair from Batch.cigars_end()
ALIGNMENT_DTYPE = np.dtype([("opsOffset", "<u8"), ("numOps", "<i4"), ("refStart", "<i4"), ("refEnd", "<i4"), ("qryStart", "<i4"),
                            ("qryEnd", "<i4"), ("matches", "<i4"), ("mismatches", "<i4"), ("insertions", "<i4"), ("deletions", "<i4"),
                            ("reserved", "<i4")])
# == struct dpx_extension (32 bytes): one record per pair from Batch.extensions()
EXTENSION_DTYPE = np.dtype([("maxScore", "<i4"), ("maxRow", "<i4"), ("maxCol", "<i4"), ("qryEndScore", "<i4"), ("qryEndCol", "<i4"),
                            ("lastDiag", "<i4"), ("flags", "<u4"), ("reserved", "<i4")])

_lib: Optional[C.CDLL] = None


def lib_path() -> str:
    """In-tree library; DPX_LIB may point at an experimental build (tools/ A-B runs)."""
    return os.environ.get("DPX_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libdpxalign.so")


def load() -> C.CDLL:
    """Load libdpxalign.so (no GPU needed just to load it).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise DpxError(-2, f"{path} is missing -- run __graft_entry__.build() (no CPU fallback exists)")
    lib = C.CDLL(path)
    vp, i32p, u32p, i16p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_int16)
    lib.dpx_init.argtypes = [C.c_int]
    lib.dpx_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.dpx_device_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    lib.dpx_pool_reserve.argtypes = [C.c_size_t, C.c_int]
    lib.dpx_text_reserve.argtypes = [C.c_size_t, C.c_int]
    lib.dpx_strerror.argtypes = [C.c_int]
    lib.dpx_strerror.restype = C.c_char_p
    lib.dpx_last_error.restype = C.c_char_p
    lib.dpx_batch_create.argtypes = [C.POINTER(Params), vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_uint,
                                     C.POINTER(vp)]
    lib.dpx_batch_create_on.argtypes = [C.c_int, C.POINTER(Params), vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_uint,
                                        C.POINTER(vp)]
    lib.dpx_pack2.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp, vp]
    lib.dpx_batch_create_packed2.argtypes = [C.c_int, C.POINTER(Params), vp, C.c_size_t, vp, vp, C.c_size_t, C.c_size_t, C.c_uint,
                                             C.POINTER(vp)]
    lib.dpx_batch_fill.argtypes = [vp, vp]
    lib.dpx_batch_fill_timed.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    lib.dpx_batch_last_fill_usec.argtypes = [vp, C.POINTER(C.c_double)]
    lib.dpx_batch_last_output_usec.argtypes = [vp, C.POINTER(C.c_double)]
    lib.dpx_batch_sync.argtypes = [vp]
    lib.dpx_batch_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.dpx_batch_results.argtypes = [vp, vp, vp, vp]
    lib.dpx_batch_matrix.argtypes = [vp, C.c_size_t, C.c_int, vp]
    lib.dpx_batch_traceback.argtypes = [vp, C.c_size_t, C.c_char_p, C.c_char_p, C.c_char_p, i32p]
    lib.dpx_batch_output_begin.argtypes = [vp, C.c_uint64]
    lib.dpx_batch_output_end.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.POINTER(C.c_uint64))]
    lib.dpx_batch_output_take.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.dpx_text_free.argtypes = [vp]
    lib.dpx_batch_info.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64)]
    lib.dpx_batch_describe.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.dpx_batch_destroy.argtypes = [vp]
    lib.dpx_align_batch.argtypes = [C.POINTER(Params), vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    lib.dpx_prim_eval.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp]
    if hasattr(lib, "dpx_batch_directions"):
        lib.dpx_batch_directions.argtypes = [vp, C.c_size_t, C.c_int, vp]
    lib.dpx_batch_cigars_begin.argtypes = [vp, C.c_uint]
    lib.dpx_batch_cigars_end.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
    lib.dpx_cigar_text.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.dpx_batch_set_extension.argtypes = [vp, C.c_int32, C.c_int32]
    lib.dpx_batch_extensions.argtypes = [vp, vp]
    lib.dpx_batch_set_substitution.argtypes = [vp, vp, C.c_int32, vp]
    lib.dpx_batch_set_extension_table.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, vp]
    lib.dpx_batch_set_direction_scoring.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, vp]
    lib.dpx_batch_set_second_gap.argtypes = [vp, C.c_int32, C.c_int32]
    lib.dpx_batch_set_reversed.argtypes = [vp, vp]
    lib.dpx_batch_set_direction_table.argtypes = [vp, vp, C.c_int32, vp]
    lib.dpx_batch_set_score_table.argtypes = [vp, vp, C.c_int32, vp]
    lib.dpx_batch_set_local_direction_table.argtypes = [vp, vp, C.c_int32, vp]
    lib.dpx_batch_diffs_begin.argtypes = [vp, C.c_uint]
    lib.dpx_batch_diffs_end.argtypes = [vp, C.c_uint, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.POINTER(C.c_uint64))]
    for name in ABI_SYMBOLS:  # every declared entry point must be exported (the optional ones by libraries that have them)
        if name not in OPTIONAL_SYMBOLS:
            getattr(lib, name)
    if lib.dpx_abi_version() < ABI_VERSION_NEEDED:
        raise DpxError(-8, f"{path} has ABI version {lib.dpx_abi_version()}, this binding needs >= {ABI_VERSION_NEEDED} -- rebuild it")
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        lib = load()
        msg = lib.dpx_strerror(rc).decode()
        detail = lib.dpx_last_error().decode()
        raise DpxError(rc, f"{what}: {msg}" + (f" [{detail}]" if detail else ""))


def init(device: int = 0) -> None:
    _check(load().dpx_init(device), "dpx_init")


def device_count() -> int:
    n = C.c_int(0)
    rc = load().dpx_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def device_info() -> Tuple[str, int, int]:
    name = C.create_string_buffer(256)
    cus, mem = C.c_int(0), C.c_size_t(0)
    _check(load().dpx_device_info(name, 256, C.byref(cus), C.byref(mem)), "dpx_device_info")
    return name.value.decode(), cus.value, mem.value


def pack2(sequences: np.ndarray, pairs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """dpx_pack2 (host only, no GPU): (packed uint8[(n+3)//4], alphabet uint8[4]) of a flat byte buffer whose pairs use at most four
    byte values; DpxError(-8) otherwise."""
    lib = load()
    seq = np.ascontiguousarray(sequences, dtype=np.uint8)
    prs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
    packed = np.zeros((seq.size + 3) // 4, np.uint8)
    alphabet = np.zeros(4, np.uint8)
    _check(lib.dpx_pack2(seq.ctypes.data, seq.size, prs.ctypes.data, len(prs), alphabet.ctypes.data, packed.ctypes.data), "dpx_pack2")
    return packed, alphabet


class Batch:
    """A device-resident batch of alignment pairs (dpx_batch).  `packed2=(packed, alphabet, num_bases)`: the sequences arrive as 2-bit
    codes (dpx_batch_create_packed2) and `sequences` is ignored."""

    def __init__(self, algo: int, sequences: np.ndarray, pairs: np.ndarray, match: int = 3, mismatch: int = -1,
                 gap_open: int = -2, gap_extend: int = -1, band: int = 0, flags: int = KEEP_MATRICES,
                 first_pair: int = 0, num_pairs: Optional[int] = None, device: int = -1, packed2=None):
        lib = load()
        self._lib = lib
        self._h = C.c_void_p(None)
        seq = np.ascontiguousarray(sequences if sequences is not None else np.zeros(0, np.uint8), dtype=np.uint8)
        prs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
        if num_pairs is None:
            num_pairs = len(prs) - first_pair
        self.params = Params(algo, match, mismatch, gap_open, gap_extend, band)
        self.pairs = prs[first_pair:first_pair + num_pairs].copy()
        self.num_pairs = num_pairs
        if packed2 is not None:
            pk = np.ascontiguousarray(packed2[0], dtype=np.uint8)
            al = np.ascontiguousarray(packed2[1], dtype=np.uint8)
            rc = lib.dpx_batch_create_packed2(device, C.byref(self.params), pk.ctypes.data, int(packed2[2]), al.ctypes.data, prs.ctypes.data,
                                              first_pair, num_pairs, flags, C.byref(self._h))
            _check(rc, "dpx_batch_create_packed2")
            return
        rc = lib.dpx_batch_create_on(device, C.byref(self.params), seq.ctypes.data, seq.size, prs.ctypes.data, first_pair,
                                     num_pairs, flags, C.byref(self._h))
        _check(rc, "dpx_batch_create")

    def fill(self, stream: int = 0) -> None:
        _check(self._lib.dpx_batch_fill(self._h, C.c_void_p(stream) if stream else None), "dpx_batch_fill")

    def fill_timed(self, repeats: int = 1) -> float:
        """Mean device microseconds of one fill over `repeats` back-to-back launches (hipEvents)."""
        us = C.c_double(0.0)
        _check(self._lib.dpx_batch_fill_timed(self._h, repeats, C.byref(us)), "dpx_batch_fill_timed")
        return us.value

    def sync(self) -> None:
        _check(self._lib.dpx_batch_sync(self._h), "dpx_batch_sync")

    def results(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        s = np.empty(self.num_pairs, np.int32)
        r = np.empty(self.num_pairs, np.int32)
        c = np.empty(self.num_pairs, np.int32)
        _check(self._lib.dpx_batch_results(self._h, s.ctypes.data, r.ctypes.data, c.ctypes.data), "dpx_batch_results")
        return s, r, c

    def device_results(self) -> Tuple[int, int, int]:
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(self._lib.dpx_batch_device_results(self._h, C.byref(a), C.byref(b), C.byref(c)),
               "dpx_batch_device_results")
        return a.value, b.value, c.value

    def matrix(self, pair: int, which: int = MAT_H) -> np.ndarray:
        m, n = int(self.pairs["querySize"][pair]), int(self.pairs["referenceSize"][pair])
        out = np.empty((m + 1, n + 1), np.int16)
        _check(self._lib.dpx_batch_matrix(self._h, pair, which, out.ctypes.data), "dpx_batch_matrix")
        return out

    def directions(self, pair: int, which: int = MAT_H) -> np.ndarray:
        """The reference's direction matrix of a KEEP_DIRECTIONS batch: uint8 (m+1, n+1), c++/backtrack.h enums (directionMain for
        MAT_H, directionIndel for ANW's MAT_I / MAT_D)."""
        if not hasattr(self._lib, "dpx_batch_directions"):
            raise DpxError(-8, f"{lib_path()} has no dpx_batch_directions -- rebuild it")
        m, n = int(self.pairs["querySize"][pair]), int(self.pairs["referenceSize"][pair])
        out = np.empty((m + 1, n + 1), np.uint8)
        _check(self._lib.dpx_batch_directions(self._h, pair, which, out.ctypes.data), "dpx_batch_directions")
        return out

    def traceback(self, pair: int) -> Tuple[str, str, str]:
        m, n = int(self.pairs["querySize"][pair]), int(self.pairs["referenceSize"][pair])
        cap = m + n + 2
        a, b, c = (C.create_string_buffer(cap) for _ in range(3))
        ln = C.c_int32(0)
        _check(self._lib.dpx_batch_traceback(self._h, pair, a, b, c, C.byref(ln)), "dpx_batch_traceback")
        k = ln.value
        return a.raw[:k].decode("latin-1"), b.raw[:k].decode("latin-1"), c.raw[:k].decode("latin-1")

    def output_begin(self, first_pair_number: int = 0) -> None:
        """Start building the batch's result text on the device (asynchronous)."""
        _check(self._lib.dpx_batch_output_begin(self._h, first_pair_number), "dpx_batch_output_begin")

    def output_end(self) -> Tuple[bytes, np.ndarray]:
        """(text, offsets): the reference's stdout blocks of every pair, and numPairs + 1 byte offsets into it."""
        text, nbytes, offs = C.c_char_p(), C.c_size_t(0), C.POINTER(C.c_uint64)()
        _check(self._lib.dpx_batch_output_end(self._h, C.byref(text), C.byref(nbytes), C.byref(offs)), "dpx_batch_output_end")
        raw = C.string_at(text, nbytes.value)
        return raw, np.ctypeslib.as_array(offs, shape=(self.num_pairs + 1,)).copy()

    def cigars_begin(self, flags: int = CIGAR_EXTENDED) -> None:
        """Start building the batch's alignment records and CIGAR ops on the device (asynchronous)."""
        _check(self._lib.dpx_batch_cigars_begin(self._h, flags), "dpx_batch_cigars_begin")

    def cigars_end(self) -> Tuple[np.ndarray, np.ndarray]:
        """(records, ops): one ALIGNMENT_DTYPE record per pair and the packed uint32 ops of the whole batch, as copies."""
        recs, ops, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        _check(self._lib.dpx_batch_cigars_end(self._h, C.byref(recs), C.byref(ops), C.byref(n)), "dpx_batch_cigars_end")
        records = np.frombuffer(C.string_at(recs, self.num_pairs * ALIGNMENT_DTYPE.itemsize), dtype=ALIGNMENT_DTYPE).copy() \
            if self.num_pairs else np.zeros(0, ALIGNMENT_DTYPE)
        out = np.frombuffer(C.string_at(ops, n.value * 4), dtype=np.uint32).copy() if n.value else np.zeros(0, np.uint32)
        return records, out

    def diffs_begin(self, kinds: int = DIFF_MD | DIFF_CS) -> None:
        """Start building the batch's MD and / or cs strings on the device (asynchronous); `kinds`: DIFF_MD, DIFF_CS or both."""
        _check(self._lib.dpx_batch_diffs_begin(self._h, kinds), "dpx_batch_diffs_begin")

    def diffs_end(self, kind: int) -> Tuple[np.ndarray, np.ndarray]:
        """(text, offsets) of one kind: the pairs' strings back to back as a uint8 array and numPairs + 1 uint64 byte offsets, as copies."""
        text, nbytes, offs = C.c_void_p(), C.c_size_t(0), C.POINTER(C.c_uint64)()
        _check(self._lib.dpx_batch_diffs_end(self._h, kind, C.byref(text), C.byref(nbytes), C.byref(offs)), "dpx_batch_diffs_end")
        raw = np.frombuffer(C.string_at(text, nbytes.value), dtype=np.uint8).copy() if nbytes.value else np.zeros(0, np.uint8)
        return raw, np.ctypeslib.as_array(offs, shape=(self.num_pairs + 1,)).copy()

    def diff_strings(self, kind: int) -> list:
        """The strings of diffs_end(kind), one bytes object per pair (cut at the offsets: a string may hold any byte)."""
        raw, offs = self.diffs_end(kind)
        data = raw.tobytes()
        return [data[int(offs[p]):int(offs[p + 1])] for p in range(self.num_pairs)]

    def set_extension(self, zdrop: int = -1, end_bonus: int = -1) -> None:
        """BAXT only: z-drop threshold and end bonus of the following fills (-1 = off; both off = plain BAXT)."""
        _check(self._lib.dpx_batch_set_extension(self._h, zdrop, end_bonus), "dpx_batch_set_extension")

    def set_substitution(self, scores, code_of=None) -> None:
        """BANW / BAXT only: score columns by scores[code_of[ref byte], code_of[qry byte]] in the following fills.

        `scores` is an int8 array of shape (A, A), 1 <= A <= 32, `code_of` 256 uint8 values below A (see code_table).  None clears the
        table.  Lines and results of an earlier fill are invalid afterwards."""
        if scores is None:
            _check(self._lib.dpx_batch_set_substitution(self._h, None, 0, None), "dpx_batch_set_substitution")
            return
        tab, code = _table_arrays(scores, code_of)
        _check(self._lib.dpx_batch_set_substitution(self._h, tab.ctypes.data, tab.shape[0], code.ctypes.data), "dpx_batch_set_substitution")

    def set_extension_table(self, zdrop: int, end_bonus: int, scores, code_of) -> None:
        """BAXT only: extension mode (set_extension's values, not both -1) and a substitution table (set_substitution's arrays, not
        None) together, the one way to have both.  Replaces both settings; lines and results of an earlier fill are invalid afterwards.
        To change a value or the table of such a batch, call this again."""
        if scores is None:
            raise ValueError("scores is required: set_extension alone runs extension mode without a table")
        tab, code = _table_arrays(scores, code_of)
        _check(self._lib.dpx_batch_set_extension_table(self._h, zdrop, end_bonus, tab.ctypes.data, tab.shape[0], code.ctypes.data),
               "dpx_batch_set_extension_table")

    def set_direction_scoring(self, zdrop: int = -1, end_bonus: int = -1, scores=None, code_of=None) -> None:
        """KEEP_BAND_DIRECTIONS batches only: all scoring at once -- z-drop and end bonus (BAXT; -1 = off) and a substitution table
        (set_substitution's arrays; None = no table).  Replaces all three settings; everything off returns the batch to k_bdir_fill.
        Lines and results of an earlier fill are invalid afterwards when a setting changed."""
        if scores is None:
            _check(self._lib.dpx_batch_set_direction_scoring(self._h, zdrop, end_bonus, None, 0, None), "dpx_batch_set_direction_scoring")
            return
        tab, code = _table_arrays(scores, code_of)
        _check(self._lib.dpx_batch_set_direction_scoring(self._h, zdrop, end_bonus, tab.ctypes.data, tab.shape[0], code.ctypes.data),
               "dpx_batch_set_direction_scoring")

    def set_direction_table(self, scores, code_of=None) -> None:
        """ANW / ASW / ASG batches created with KEEP_DIRECTIONS only: score columns by scores[code_of[ref byte], code_of[qry byte]] in the
        following fills (set_substitution's arrays; the table need not be symmetric).  None clears the table.  Lines and results of an
        earlier fill are invalid afterwards when the table changed."""
        if scores is None:
            _check(self._lib.dpx_batch_set_direction_table(self._h, None, 0, None), "dpx_batch_set_direction_table")
            return
        tab, code = _table_arrays(scores, code_of)
        _check(self._lib.dpx_batch_set_direction_table(self._h, tab.ctypes.data, tab.shape[0], code.ctypes.data), "dpx_batch_set_direction_table")

    def set_score_table(self, scores, code_of=None) -> None:
        """ANW / ASW / ASG batches created with SCORE_ONLY only: score columns by scores[code_of[ref byte], code_of[qry byte]] in the
        following fills (set_substitution's arrays; the table need not be symmetric).  None clears the table.  Results of an earlier
        fill are invalid afterwards when the table changed."""
        if scores is None:
            _check(self._lib.dpx_batch_set_score_table(self._h, None, 0, None), "dpx_batch_set_score_table")
            return
        tab, code = _table_arrays(scores, code_of)
        _check(self._lib.dpx_batch_set_score_table(self._h, tab.ctypes.data, tab.shape[0], code.ctypes.data), "dpx_batch_set_score_table")

    def set_local_direction_table(self, scores, code_of=None) -> None:
        """BSW / BASW batches created with KEEP_LOCAL_BAND_DIRECTIONS (band not covering) only: score columns by
        scores[code_of[ref byte], code_of[qry byte]] in the following fills (set_substitution's arrays; the table need not be symmetric).
        None clears the table.  Lines and results of an earlier fill are invalid afterwards when the table changed.  A
        LOCAL_TWO_PIECE_GAPS batch takes the same setter."""
        if scores is None:
            _check(self._lib.dpx_batch_set_local_direction_table(self._h, None, 0, None), "dpx_batch_set_local_direction_table")
            return
        tab, code = _table_arrays(scores, code_of)
        _check(self._lib.dpx_batch_set_local_direction_table(self._h, tab.ctypes.data, tab.shape[0], code.ctypes.data),
               "dpx_batch_set_local_direction_table")

    def set_second_gap(self, gap_open2: int, gap_extend2: int) -> None:
        """TWO_PIECE_GAPS and LOCAL_TWO_PIECE_GAPS batches only: the second gap piece of the following fills; a gap of length k then scores
        max(gap_open + k * gap_extend, gap_open2 + k * gap_extend2).  Lines and results of an earlier fill are invalid afterwards when a
        value changed."""
        _check(self._lib.dpx_batch_set_second_gap(self._h, gap_open2, gap_extend2), "dpx_batch_set_second_gap")

    def set_reversed(self, mask) -> None:
        """BANW / BAXT only: the pairs whose mask entry is nonzero are aligned as (reverse(ref), reverse(qry)) in the following fills,
        on the device.  Results, extension records and exported planes stay in that reversed frame; lines, text, CIGAR ops and alignment
        coordinates come back in the original orientation.  `mask` holds num_pairs values; None or all zeros clears it.  Lines and
        results of an earlier fill are invalid afterwards."""
        if mask is None:
            _check(self._lib.dpx_batch_set_reversed(self._h, None), "dpx_batch_set_reversed")
            return
        arr = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        if arr.size != self.num_pairs:
            raise ValueError(f"mask must hold one value per pair ({self.num_pairs}), got {arr.size}")
        _check(self._lib.dpx_batch_set_reversed(self._h, arr.ctypes.data if arr.size else None), "dpx_batch_set_reversed")

    def extensions(self) -> np.ndarray:
        """One EXTENSION_DTYPE record per pair of the last fill, which must have run in extension mode."""
        out = np.zeros(self.num_pairs, EXTENSION_DTYPE)
        _check(self._lib.dpx_batch_extensions(self._h, out.ctypes.data), "dpx_batch_extensions")
        return out

    def info(self) -> dict:
        npairs, cells, mb, ab = C.c_size_t(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(self._lib.dpx_batch_info(self._h, C.byref(npairs), C.byref(cells), C.byref(mb), C.byref(ab)),
               "dpx_batch_info")
        return {"num_pairs": npairs.value, "cells": cells.value, "matrix_bytes": mb.value,
                "algorithmic_bytes": ab.value}

    def describe(self) -> dict:
        """How the engine fills this batch (dpx_batch_describe): kernel, arithmetic type, launch-list sizes."""
        buf = C.create_string_buffer(2048)
        _check(self._lib.dpx_batch_describe(self._h, buf, 2048), "dpx_batch_describe")
        out = dict(kv.split("=", 1) for kv in buf.value.decode().split())
        return {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in out.items()}

    def close(self) -> None:
        if self._h and self._h.value:
            self._lib.dpx_batch_destroy(self._h)
            self._h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _table_arrays(scores, code_of):
    """(int8 (A, A) table, uint8 (256,) map) as contiguous arrays, or ValueError: the argument checking of the two table setters"""
    tab = np.ascontiguousarray(scores, dtype=np.int8)
    if tab.ndim != 2 or tab.shape[0] != tab.shape[1] or not np.array_equal(tab, np.asarray(scores)):
        raise ValueError("scores must be a square matrix of int8 values")
    if code_of is None:
        raise ValueError("code_of is required with a table")
    code = np.ascontiguousarray(code_of, dtype=np.uint8)
    if code.shape != (256,) or not np.array_equal(code, np.asarray(code_of).reshape(-1)):
        raise ValueError("code_of must hold 256 values in 0..255")
    return tab, code


def code_table(alphabet: bytes, fold_case: bool = True) -> np.ndarray:
    """The 256-entry byte -> code map of Batch.set_substitution for `alphabet`: letter k gets code k, every unlisted byte the code of the
    LAST letter ('N' of b"ACGTN", '*' of an NCBI protein alphabet).  fold_case: a lower-case byte takes its upper-case letter's code."""
    letters = bytes(alphabet)
    if not 1 <= len(letters) <= 32 or len(set(letters)) != len(letters):
        raise ValueError("alphabet must hold 1..32 distinct bytes")
    code = np.full(256, len(letters) - 1, np.uint8)
    for k, ch in enumerate(letters):
        code[ch] = k
    if fold_case:
        for lo in range(ord("a"), ord("z") + 1):
            up = lo - 32
            if lo not in letters and up in letters:
                code[lo] = code[up]
    return code


def cigar_text(ops) -> str:
    """SAM text of an array of ops (dpx_cigar_text; host only, no GPU): "12=1X3D", "*" for none."""
    lib = load()
    arr = np.ascontiguousarray(ops, dtype=np.uint32)
    cap = 11 * arr.size + 2  # at most ten digits and a letter per op
    buf = C.create_string_buffer(cap)
    n = C.c_size_t(0)
    _check(lib.dpx_cigar_text(arr.ctypes.data if arr.size else None, arr.size, buf, cap, C.byref(n)), "dpx_cigar_text")
    return buf.raw[:n.value].decode("ascii")


def prim_eval(ops: Sequence[int], a: Sequence[int], b: Sequence[int], c: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """Evaluate DPX primitives on the device (dpx_prim_eval).  Returns (result, pred)."""
    op = np.ascontiguousarray(ops, np.int32)
    A = np.ascontiguousarray(np.asarray(a, np.uint64) & 0xFFFFFFFF, np.uint32)
    B = np.ascontiguousarray(np.asarray(b, np.uint64) & 0xFFFFFFFF, np.uint32)
    Cc = np.ascontiguousarray(np.asarray(c, np.uint64) & 0xFFFFFFFF, np.uint32)
    res = np.empty(len(op), np.uint32)
    pred = np.empty(len(op), np.uint32)
    _check(load().dpx_prim_eval(op.ctypes.data, A.ctypes.data, B.ctypes.data, Cc.ctypes.data, len(op),
                                res.ctypes.data, pred.ctypes.data), "dpx_prim_eval")
    return res, pred
