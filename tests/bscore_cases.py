"""The inputs and expectations of the DPX_LONG_SCORES tests (tests/test_gpu_bscore.py, tests/test_gpu_bscore_drivers.py).  TEST
INFRASTRUCTURE ONLY -- never imported by the product.  Pure CPU: the pair sets, and what the int64 band-only oracles (tests/bdx_oracle.c,
bdl_oracle.c, bdlt_oracle.c, through their reference helpers as they are) say about them."""
import numpy as np

import bdl_ref
import bdlt_ref
import bdx_ref
import zsub_ref

BANW, BAXT, BSW, BASW = 7, 10, 3, 5
ALGOS = (BANW, BAXT, BSW, BASW)
NAME = {BANW: "BANW", BAXT: "BAXT", BSW: "BSW", BASW: "BASW"}
KERNEL = {BANW: "k_bscore_fill", BAXT: "k_bscore_fill", BSW: "k_lscore_fill", BASW: "k_lscore_fill"}
TWIN_KERNELS = {BANW: ("k_bdir_fill", "k_bdx_fill"), BAXT: ("k_bdir_fill", "k_bdx_fill"), BSW: ("k_bdl_fill", "k_bdlt_fill"), BASW: ("k_bdl_fill", "k_bdlt_fill")}
W = (2, -4, -4, -2)  # the weights at which the int16 DPX_SCORE_ONLY batch admits 300 - 600 bases
BANDS = (1, 2, 33, 64, 65, 128, 129, 255, 256, 257, 511, 512)  # every C class, both parities, both sides of each class boundary
ACGT = np.frombuffer(b"ACGT", np.uint8)
ZDROPPED, REACHED_END = 1, 2


def is_local(algo):
    return algo in (BSW, BASW)


def weights(algo, w=W):
    """the batch's four weights: BSW has one linear gap weight"""
    return (w[0], w[1], w[2], w[3] if algo != BSW else 0)


class Oracles:
    """the three band-only oracles, built once"""

    def __init__(self, out_dir):
        self.bdx, self.bdl, self.bdlt = bdx_ref.build(out_dir), bdl_ref.build(out_dir), bdlt_ref.build(out_dir)

    def expect(self, algo, ref, qry, band, w=W, table=None, zdrop=-1, end_bonus=-1, used=b"ACGTN"):
        """(score, (end row, end column), record or None) of one pair.  table = (scores, code_of) or None (byte equality by w)"""
        if not is_local(algo):
            t, c = table if table is not None else bdx_ref.byte_table(w[0], w[1], used)
            r = self.bdx.fill(ref, qry, t, c, w[2], w[3], band, algo == BAXT, zdrop, end_bonus)
            return r["score"], r["end"], (r["rec"] if (zdrop >= 0 or end_bonus >= 0) else None)
        if table is None:
            r = self.bdl.align(algo, ref, qry, w, band)
        else:
            r = self.bdlt.align(algo, ref, qry, table, bdlt_ref.gaps(algo, (w[2], w[3])), band)
        return int(r["score"]), tuple(r["end"]), None

    def expect_all(self, algo, texts, band, **kw):
        return [self.expect(algo, ref, qry, band, **kw) for ref, qry in texts]


def mutated(rng, ref, m, subs=0.08, indels=3):
    """a copy of `ref` (codes 0..3) with about 8 % substitutions and a few short insertions and deletions, cut or padded to m bases"""
    q = ref.copy()
    sub = rng.random(len(q)) < subs
    q[sub] = rng.integers(0, 4, int(sub.sum()))
    for _ in range(indels if len(q) > 8 else 0):
        at = int(rng.integers(0, len(q) + 1))
        q = np.concatenate([q[:at], rng.integers(0, 4, int(rng.integers(1, 3))), q[at:]])
        at = int(rng.integers(0, max(len(q) - 2, 1)))
        q = np.concatenate([q[:at], q[at + int(rng.integers(1, 3)):]])
    q = q[:m]
    return np.concatenate([q, rng.integers(0, 4, m - len(q))])


def related(rng, m, n, **kw):
    """(reference of n bases, query of m bases that is a mutated copy of it)"""
    ref = rng.integers(0, 4, n)
    return ACGT[ref].tobytes(), ACGT[mutated(rng, ref, m, **kw)].tobytes()


def unrelated(rng, m, n):
    return ACGT[rng.integers(0, 4, n)].tobytes(), ACGT[rng.integers(0, 4, m)].tobytes()


def band_pairs(algo, band):
    """About 64 (reference, query) texts for one batch at `band`: lengths B + 40 .. 2B + 90, unequal, so that the head, interior and tail
    phases all run (BANW: |m - n| of 0, 1 and B - 1 among them, every pair inside its admission rule |m - n| < B); and the degenerate
    shapes: m or n in {0, 1, 2}, m + n - 1 odd and even, pairs shorter than the band."""
    rng = np.random.default_rng(1000 * algo + band)
    lo, hi = band + 40, 2 * band + 90
    texts = []
    banw_diffs = [d for d in (0, 1, -1, band - 1, -(band - 1)) if abs(d) < band]
    for k in range(44):
        m = int(rng.integers(lo, hi + 1))
        if algo == BANW:
            d = banw_diffs[k % len(banw_diffs)] if k < 15 else int(rng.integers(-(band - 1), band))
            n = m + d  # (at least 41 bases: m >= B + 40 and d > -B)
        else:
            n = int(rng.integers(lo, hi + 1))
            n = n + 1 if n == m else n
        texts.append(related(rng, m, n) if k % 4 else unrelated(rng, m, n))
    small = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1), (1, 2), (2, 1), (2, 2), (0, 5), (5, 0), (1, 7), (7, 1), (2, 9), (9, 2),
             (1, band + 40), (band + 41, 2), (0, band + 40), (band + 40, 0)]
    short = [(max(band // 2, 1), max(band // 2, 1)), (max(band // 3, 1), max(band // 3, 1) + 1), (max(band - 1, 1), max(band - 2, 1))]
    for m, n in small + short:
        if algo == BANW and abs(m - n) >= band:
            continue
        texts.append(related(rng, m, n) if min(m, n) > 2 else unrelated(rng, m, n))
    assert all(algo != BANW or abs(len(q) - len(r)) < band for r, q in texts)
    return texts


def extension_pairs(seed=5, count=24):
    """BAXT's extension set: pairs related for a prefix and unrelated behind it, next to fully related pairs (m, n around 300 - 420)"""
    rng = np.random.default_rng(seed)
    texts = []
    for k in range(count):
        m, n = int(rng.integers(300, 400)), int(rng.integers(300, 420))
        if k % 2:
            texts.append(related(rng, m, n, subs=0.04))
        else:
            pre = int(rng.integers(60, 200))
            ref, qry = related(rng, pre, pre, subs=0.03, indels=1)
            tail = unrelated(rng, m - pre, n - pre)
            texts.append((ref + tail[0], qry + tail[1]))
    texts += [(b"", b"ACGTACGT"), (b"ACGTAC", b""), (b"A", b"A")]
    return texts


def long_pairs():
    """[(reference, query, band)]: 33 000 x 33 000 at band 64, and 20 000 x 20 300 at band 256 with eight planted indels of 100 - 250
    bases, alternating, so that the path swings across the band"""
    rng = np.random.default_rng(77)
    ref = rng.integers(0, 4, 33000)
    a = (ACGT[ref].tobytes(), ACGT[mutated(rng, ref, 33000, subs=0.05, indels=20)].tobytes(), 64)
    ref = rng.integers(0, 4, 20300)
    q, at = ref.copy(), 1500
    for k in range(8):
        size = int(rng.integers(100, 251))
        q = np.concatenate([q[:at], q[at + size:]]) if k % 2 == 0 else np.concatenate([q[:at], rng.integers(0, 4, size), q[at:]])
        at += 2200
    q = np.concatenate([q, rng.integers(0, 4, 20000)])[:20000]
    return [a, (ACGT[ref].tobytes(), ACGT[q].tobytes(), 256)]


def high_table():
    """a 4-code table whose entries all lie in 100 .. 127 (asymmetric), over ACGT; every other byte takes code 3"""
    rng = np.random.default_rng(3)
    tab = rng.integers(100, 128, (4, 4)).astype(np.int8)
    tab[0, 1], tab[1, 0] = 100, 127
    code = np.full(256, 3, np.uint8)
    for k, ch in enumerate(b"ACGT"):
        code[ch] = k
    return tab, code


def acgtn_pairs(seed=11, count=32, lo=150, hi=260):
    """pairs over ACGTN (about 3 % N) with lower-case stretches, for the 5 x 5 tables"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        m = int(rng.integers(lo, hi))
        n = m + int(rng.integers(-40, 41))
        ref, qry = related(rng, m, n)
        ref, qry = bytearray(ref), bytearray(qry)
        for s in (ref, qry):
            for at in np.nonzero(rng.random(len(s)) < 0.03)[0]:
                s[at] = ord("N")
            a = int(rng.integers(0, max(len(s) - 20, 1)))
            s[a:a + 20] = bytes(s[a:a + 20]).lower()
        out.append((bytes(ref), bytes(qry)))
    return out


def byte_pairs(seed=12, count=32, lo=150, hi=260):
    """pairs over all 256 byte values (bytes >= 128 included), related through a 12 % substitution, for the 32-code table"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        m = int(rng.integers(lo, hi))
        n = m + int(rng.integers(-40, 41))
        ref = rng.integers(1, 256, n).astype(np.uint8)  # (0 separates the strings in the flat buffer's text form; no kernel cares)
        qry = np.resize(ref, m).copy()
        sub = rng.random(m) < 0.12
        qry[sub] = rng.integers(1, 256, int(sub.sum()))
        out.append((ref.tobytes(), qry.tobytes()))
    return out


ACGTN_TABLE = zsub_ref.acgtn_table()              # 5 x 5 with a negative N-N and one asymmetric entry
WIDE_TABLE = bdlt_ref.random_table(41)            # asymmetric, 32 codes, holds -128 and 127, maps every byte
