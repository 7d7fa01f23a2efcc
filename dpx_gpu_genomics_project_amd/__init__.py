"""dpx_gpu_genomics_project_amd -- MI355X-native pairwise-alignment DP engine (hot path only).

The product is ``libdpxalign.so`` (hand-written HIP kernels for gfx950 behind the C ABI of
``include/dpx_align.h``) plus the C++ host mirror of the reference's class surface in ``hostcpp/``.
This Python package is plumbing: a ctypes binding of the C ABI (used by tests/ and bench.py) and the
synthetic-input generator.  There is no CPU fallback: every compute call raises ``DpxError`` when the
library or a GPU is missing.
"""
from .capi import (  # noqa: F401
    ALGO_ANW,
    ALGO_ASG,
    ALGO_ASW,
    ALGO_BANW,
    ALGO_BASW,
    ALGO_BAXT,
    ALGO_BSW,
    ALGO_LNW,
    ALGO_LSW,
    ALGO_NAMES,
    ALIGNMENT_DTYPE,
    CIGAR_EXTENDED,
    CIGAR_M,
    CIGAR_OP_D,
    CIGAR_OP_EQ,
    CIGAR_OP_I,
    CIGAR_OP_M,
    CIGAR_OP_X,
    DIFF_CS,
    DIFF_MD,
    EXT_NO_QUERY_END,
    EXT_REACHED_END,
    EXT_ZDROPPED,
    EXTENSION_DTYPE,
    MAT_D,
    MAT_H,
    MAT_I,
    MAT_D2,
    MAT_H_PIECE,
    MAT_I2,
    TWO_PIECE_GAPS,
    LOCAL_TWO_PIECE_GAPS,
    LONG_SCORES,
    SCORE_ONLY,
    TIME_FILLS,
    TUNE_PLACEMENT,
    KEEP_MATRICES,
    KEEP_BAND_DIRECTIONS,
    KEEP_LOCAL_BAND_DIRECTIONS,
    KEEP_DIRECTIONS,
    Batch,
    DpxError,
    Params,
    SeqPair,
    cigar_text,
    code_table,
    device_count,
    device_info,
    init,
    lib_path,
    load,
    pack2,
    prim_eval,
)
from .synth import SynthBatch, make_batch, parse_pairs_file, write_pairs_file  # noqa: F401

__all__ = [
    "ALGO_ANW", "ALGO_ASG", "ALGO_ASW", "ALGO_BANW", "ALGO_BASW", "ALGO_BAXT", "ALGO_BSW", "ALGO_LNW", "ALGO_LSW", "ALGO_NAMES", "MAT_D", "MAT_H", "MAT_I", "SCORE_ONLY", "TIME_FILLS", "TUNE_PLACEMENT",
    "KEEP_MATRICES", "KEEP_DIRECTIONS", "KEEP_BAND_DIRECTIONS", "KEEP_LOCAL_BAND_DIRECTIONS", "TWO_PIECE_GAPS", "LOCAL_TWO_PIECE_GAPS", "LONG_SCORES", "MAT_I2", "MAT_D2", "MAT_H_PIECE", "Batch", "DpxError", "Params", "SeqPair", "device_count", "device_info", "init",
    "lib_path", "load", "pack2", "prim_eval", "ALIGNMENT_DTYPE", "CIGAR_EXTENDED", "CIGAR_M", "CIGAR_OP_D", "CIGAR_OP_EQ", "CIGAR_OP_I",
    "CIGAR_OP_M", "CIGAR_OP_X", "DIFF_CS", "DIFF_MD", "cigar_text", "code_table", "EXT_NO_QUERY_END", "EXT_REACHED_END", "EXT_ZDROPPED", "EXTENSION_DTYPE", "SynthBatch", "make_batch", "parse_pairs_file", "write_pairs_file",
]
