"""The same strings under different flat-buffer layouts.  TEST INFRASTRUCTURE ONLY -- never imported by the product, plain numpy, no GPU.

include/dpx_align.h puts no constraint on where a batch's strings sit: dpx_seq_pair holds byte offsets into the flat buffer, firstPair
selects a slice of the pair table and any byte value is legal.  synth.from_strings / make_batch / make_ragged_batch give every test one
layout -- `head\\0 ref \\0 qry \\0` in ascending order, the window starting at byte 0, a NUL on both sides of every string -- so a read one
byte past either string always compares NUL with NUL.  lay(layout, texts) re-lays [(ref, qry), ...] without changing a byte of them:

  canonical       synth.from_strings (the control)
  residues        test_gpu_reversed._flat's placement (pair p's reference on residue p, its query on p + 8, modulo 16) with filler
                  instead of NULs, the whole behind 5 more filler bytes: the smallest used offset is 5, so the uploaded window starts
                  there and device residues (p, p + 8) differ from host residues (p + 5, p + 13)
  tight_reversed  no byte between two strings, pairs last to first, the query before the reference: offsets descend, queryIdx <
                  referenceIdx, and pair 0's reference ends on the buffer's last byte
  embedded        every string is the inner slice of a longer one, 40 bytes before and 40 after, and a pair's reference and query have
                  the SAME flanks: a read past either end of both strings sees a perfect continuation of the alignment.  Laid.outer(p)
                  gives the strings with their flanks
  shared          strings are stored once: equal references share one copy, a query equal to its reference has queryIdx ==
                  referenceIdx, a query that is a substring of its reference points inside it, nothing separates the copies; a pair
                  that repeats an earlier pair's texts gets an identical record
  windowed        the `residues` placement behind 4096 + 5 junk bytes (smallest used offset 4101), two decoy pairs before and two
                  after the real ones in the table (other lengths, pointing into the junk); the batch is first_pair=2, num_pairs=len(texts)

Filler, flanks and junk are never NUL: they cycle through the bytes that occur in the texts (ACGT where all are empty), so a stray read
scores like real sequence.  Laid.coverage is the set of (kind, device residue) of the non-empty strings, kind "ref" or "qry", residue =
(offset - smallest used offset) mod 16: what stage_bytes / load4 / CharWin / load_query_rows see on the byte path."""
from dataclasses import dataclass, field

import numpy as np

from dpx_gpu_genomics_project_amd.capi import PAIR_DTYPE
from dpx_gpu_genomics_project_amd.synth import SynthBatch, from_strings

LAYOUTS = ("canonical", "residues", "tight_reversed", "embedded", "shared", "windowed")
FLANK = 40
LEAD = 5
JUNK = 4096 + LEAD
DECOYS_BEFORE = [(10, 33, 60, 29), (100, 9, 300, 0)]         # (referenceIdx, referenceSize, queryIdx, querySize), inside the junk
DECOYS_AFTER = [(200, 50, 1000, 45), (4000, 61, 2000, 3)]


@dataclass
class Laid:
    layout: str
    sequences: np.ndarray          # uint8, the whole flat buffer
    pairs: np.ndarray              # PAIR_DTYPE, the whole table (decoys included)
    first_pair: int = 0
    num_pairs: int = 0
    outers: list = field(default_factory=list)   # embedded only: [(reference with flanks, query with flanks)]

    @property
    def sb(self) -> SynthBatch:
        """the batch's own pairs over the whole buffer: ref(p) / qry(p) are the texts"""
        own = self.pairs[self.first_pair:self.first_pair + self.num_pairs]
        return SynthBatch(self.sequences, own, int(own["querySize"].max(initial=0)), int(own["referenceSize"].max(initial=0)))

    @property
    def kwargs(self) -> dict:
        """first_pair / num_pairs for Batch(algo, laid.sequences, laid.pairs, ...)"""
        return {"first_pair": self.first_pair, "num_pairs": self.num_pairs}

    @property
    def smallest_offset(self) -> int:
        own = self.sb.pairs
        return int(min(own["referenceIdx"].min(), own["queryIdx"].min())) if len(own) else 0

    @property
    def coverage(self) -> set:
        own, lo = self.sb.pairs, self.smallest_offset
        return {(kind, (int(r[idx]) - lo) % 16) for r in own for kind, idx, size in (("ref", "referenceIdx", "referenceSize"), ("qry", "queryIdx", "querySize"))
                if r[size] > 0}

    def outer(self, p):
        return self.outers[p]


class _Filler:
    """an endless cycle through the distinct bytes of the texts; never NUL"""

    def __init__(self, texts):
        letters = sorted(set(b"".join(r + q for r, q in texts)) - {0}) or list(b"ACGT")
        self.letters, self.at = bytes(letters), 0

    def take(self, count: int) -> bytes:
        out = bytes(self.letters[(self.at + k) % len(self.letters)] for k in range(count))
        self.at += count
        return out


def _bytes(texts):
    return [(r.encode("latin-1") if isinstance(r, str) else bytes(r), q.encode("latin-1") if isinstance(q, str) else bytes(q)) for r, q in texts]


def _table(records):
    pairs = np.zeros(len(records), PAIR_DTYPE)
    for p, rec in enumerate(records):
        pairs[p] = rec
    return pairs


def _laid(layout, buf, records, **kw):
    return Laid(layout, np.frombuffer(bytes(buf), np.uint8).copy(), _table(records), num_pairs=kw.pop("num_pairs", len(records)), **kw)


def _residues(texts, fill, lead):
    """`lead` filler bytes, then pair p's reference at lead + (p mod 16) and its query at lead + (p + 8 mod 16), modulo 16"""
    buf, records = bytearray(fill.take(lead)), []
    for p, (ref, qry) in enumerate(texts):
        at = []
        for side, s in enumerate((ref, qry)):
            buf += fill.take(((p + 8 * side) - (len(buf) - lead)) % 16)
            at.append(len(buf))
            buf += s
        records.append((at[0], len(ref), at[1], len(qry)))
    return buf, records


def _tight_reversed(texts, fill):
    buf, records = bytearray(), [None] * len(texts)
    for p in reversed(range(len(texts))):
        ref, qry = texts[p]
        records[p] = (len(buf) + len(qry), len(ref), len(buf), len(qry))
        buf += qry + ref
    return (buf or bytearray(fill.take(1))), records


def _embedded(texts, fill):
    buf, records, outers = bytearray(), [], []
    for ref, qry in texts:
        before, after = fill.take(FLANK), fill.take(FLANK)
        at = []
        for s in (ref, qry):
            at.append(len(buf) + FLANK)
            buf += before + s + after
        records.append((at[0], len(ref), at[1], len(qry)))
        outers.append((before + ref + after, before + qry + after))
    return buf, records, outers


def _shared(texts, fill):
    buf, records, placed = bytearray(), [], {}

    def place(s):
        if s not in placed:
            placed[s] = len(buf)
            buf.extend(s)
        return placed[s]

    for ref, qry in texts:
        r = place(ref)
        q = r if qry == ref else r + ref.find(qry) if qry and qry in ref else place(qry)
        records.append((r, len(ref), q, len(qry)))
    return (buf or bytearray(fill.take(1))), records


def lay(layout: str, texts) -> Laid:
    texts = _bytes(texts)
    fill = _Filler(texts)
    if layout == "canonical":
        sb = from_strings(texts)
        return Laid(layout, sb.sequences, sb.pairs, num_pairs=len(texts))
    if layout == "residues":
        return _laid(layout, *_residues(texts, fill, LEAD))
    if layout == "tight_reversed":
        return _laid(layout, *_tight_reversed(texts, fill))
    if layout == "embedded":
        buf, records, outers = _embedded(texts, fill)
        return _laid(layout, buf, records, outers=outers)
    if layout == "shared":
        return _laid(layout, *_shared(texts, fill))
    if layout == "windowed":
        buf, records = _residues(texts, fill, JUNK)
        return _laid(layout, buf, DECOYS_BEFORE + records + DECOYS_AFTER, first_pair=len(DECOYS_BEFORE), num_pairs=len(texts))
    raise ValueError(layout)


def texts_of(sb: SynthBatch):
    """the texts of a batch made by synth (to re-lay make_ragged_batch's pairs)"""
    return [(sb.ref(p), sb.qry(p)) for p in range(sb.num_pairs)]
