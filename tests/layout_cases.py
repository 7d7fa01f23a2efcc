"""The case table of tests/test_layouts.py (CPU: planner invariance, the oracle-only assertions) and tests/test_gpu_layouts.py (GPU: every
fill kernel under every layout of tests/layouts.py).  TEST INFRASTRUCTURE ONLY -- never imported by the product.

One small batch per fill kernel of dpx_route_kernel_name, forced the way the kernel's own GPU test forces it, and for each the CPU oracle
of its algorithm -- the ones those tests use.  An expectation depends on the texts only: want() computes it once per case and every
layout, walk and test shares it.  Behind the storing cases come the DPX_SCORE_ONLY cases -- every route such a batch can take, each on
the texts, the oracle and the want() of its storing sibling -- and the table twins of ANW / ASW / ASG (dpx_batch_set_score_table on the
score-only cases, dpx_batch_set_direction_table on the direction cases, tests/dirtab_ref.py), which launch under unchanged kernel= names.

TEXTS (standard_texts): 18 ACGT pairs, lengths 0, 1, 15, 16, 17, 63, 64, 65 and 131 among them, |m - n| < 17 so that BANW admits them at
band 17, longest string 131 so that no band of 129 covers the batch.  Pairs 0..2 share one reference of 131 (a mutated query, a query
that is a slice of that reference, a query equal to it), pair 13 repeats pair 12, pairs 16 and 17 have the empty reference and the empty
query -- on residues that pairs 0 and 1 cover as well, so the 16 non-empty references and 16 non-empty queries in front of them put a
string of each kind on every residue."""
from dataclasses import dataclass, field, replace

import numpy as np

import asg_ref
import asw_ref
import banw_ref
import basw_ref
import baxt_ref
import bd2_ref
import bdl_ref
import bdx_ref
import dirtab_ref
import layouts
import subst_ref
import zext_ref
import zsub_ref
from dpx_gpu_genomics_project_amd import capi
from dpx_gpu_genomics_project_amd.synth import make_ragged_batch
from test_gpu_banddir import want_directions
from test_gpu_poison import KNOBS, _dir_global, _expect

ACGT = np.frombuffer(b"ACGT", np.uint8)
LIN, AFF, HARSH = (3, -1, -2), (3, -1, -3, -1), (2, -3, -5, -1)
TABLE, CODE = zsub_ref.acgtn_table()
GAPS = zsub_ref.GAPS                     # (-5, -1), with the table
MM = (2, -3)                             # params.match / mismatch of the table-less band-direction modes
P1, P2 = (-4, -2), (-24, -1)             # the two gap pieces (tests/test_gpu_bd2.py)
Z, E = 20, 5
CODE_OF = {"LNW": 0, "LSW": 1, "ANW": 2, "BSW": 3, "ASW": 4, "BASW": 5, "ASG": 6, "BANW": 7, "BAXT": 10}
FLAGS = {"mat": capi.KEEP_MATRICES, "dirs": capi.KEEP_DIRECTIONS, "bdirs": capi.KEEP_BAND_DIRECTIONS,
         "two": capi.KEEP_BAND_DIRECTIONS | capi.TWO_PIECE_GAPS, "local": capi.KEEP_LOCAL_BAND_DIRECTIONS, "score": capi.SCORE_ONLY}
BANDS = (17, 129)                        # 1 and 4 cells per lane
LOCAL_OR_EXTENSION = ("LSW", "BSW", "ASW", "BASW", "ASG", "BAXT")   # (ASG: free reference ends)
KERNELS = {"k_linear_fill", "k_linear_fill_pk", "k_linear_lanes", "k_linear_lanes_pk", "k_linear_split", "k_affine_fill", "k_asw_fill",
           "k_asg_fill", "k_affine_lanes", "k_asw_lanes", "k_asg_lanes", "k_banded_fill", "k_banded_fill_pk", "k_basw_fill", "k_banw_fill",
           "k_baxt_fill", "k_zext_fill", "k_subst_fill", "k_zsub_fill", "k_bdir_fill", "k_bdx_fill", "k_bd2_fill", "k_linear_dir",
           "k_affine_dir", "k_asw_dir", "k_asg_dir", "k_bdl_fill"}      # dpx_route_kernel_name, csrc/dpx_plan.cpp


# ----------------------------------------------------------------------------------------------------------------------- texts

def _mutated(rng, ref: bytes, m: int) -> bytes:
    """a query of m bytes related to `ref` over its whole length: 8 % substitutions, one deletion and one insertion where there is room"""
    q = np.frombuffer(ref, np.uint8).copy()
    sub = rng.random(q.size) < 0.08
    q[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
    if q.size > 20:
        q = np.delete(q, int(rng.integers(5, q.size - 5)))
        q = np.insert(q, int(rng.integers(5, q.size - 5)), ACGT[rng.integers(0, 4)])
    if q.size >= m:
        return q[:m].tobytes()
    return np.concatenate([q, ACGT[rng.integers(0, 4, m - q.size)]]).tobytes()


def _random(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def standard_texts(seed=7):
    rng = np.random.default_rng(seed)
    big = _random(rng, 131)
    out = [(big, _mutated(rng, big, 125)), (big, big[3:123]), (big, big)]
    for n, m in ((1, 1), (15, 16), (16, 15), (17, 17), (63, 64), (64, 63), (65, 65)):
        ref = _random(rng, n)
        out.append((ref, _mutated(rng, ref, m)))
    ref = _random(rng, 16)
    out.append((ref, ref))
    ref = _random(rng, 64)
    out.append((ref, ref[2:62]))
    ref = _random(rng, 40)
    out += [(ref, _mutated(rng, ref, 45))] * 2
    for n, m in ((33, 30), (100, 90)):
        ref = _random(rng, n)
        out.append((ref, _mutated(rng, ref, m)))
    return out + [(b"", _random(rng, 5)), (_random(rng, 7), b"")]


def coupled_texts(seed=11):
    """k_linear_fill_pk couples pairs of one shape: nine shapes twice and one left over (19 pairs, an odd count: couples and a single),
    among them a query equal to its reference, a query that is a slice of it and, behind the 16 pairs that put a non-empty string of
    each kind on every residue, the empty reference and the empty query"""
    rng = np.random.default_rng(seed)
    out = []
    for n, m in ((1, 1), (16, 15), (17, 17), (63, 64), (64, 65), (130, 65)):
        for _ in range(2):
            ref = _random(rng, n)
            out.append((ref, _mutated(rng, ref, m)))
    for _ in range(2):
        ref = _random(rng, 70)
        out.append((ref, ref))
    for _ in range(2):
        ref = _random(rng, 90)
        out.append((ref, ref[10:70]))
    return out + [(b"", _random(rng, 5))] + [(_random(rng, 5), b"") for _ in range(2)]


def split_texts():
    """k_linear_split takes no empty pair (the planner then leaves the batch to k_linear_fill): the 16 non-empty pairs of the standard
    texts, whose longest query of 131 makes two stripes of 128 rows"""
    return standard_texts()[:16]


def ragged_couples_texts(seed=41):
    """k_banded_fill_pk runs couples of equal-shaped pairs only, which make_ragged_batch(40, ...) does not have: 20 shapes drawn from
    its ranges (m 1..256, n 1..260), each twice with different bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(20):
        n, m = int(rng.integers(1, 261)), int(rng.integers(1, 257))
        for _ in range(2):
            ref = _random(rng, n)
            out.append((ref, _mutated(rng, ref, m)))
    return out


def ragged40_texts():
    return layouts.texts_of(make_ragged_batch(40, 1, 256, 1, 260, seed=40))


def ragged40_acgt_texts():
    """the same 40 pairs in the letters ACGT: under the five-letter table the digits would all be N"""
    digits = bytes.maketrans(b"0123", b"ACGT")
    return [(ref.translate(digits), qry.translate(digits)) for ref, qry in ragged40_texts()]


def global_edge_texts(nedges):
    return layouts.texts_of(_dir_global(nedges))


_TEXTS = {}


def texts_of(case):
    key = (case.texts.__name__, case.texts_args)
    if key not in _TEXTS:
        _TEXTS[key] = case.texts(*case.texts_args)
    return _TEXTS[key]


# ----------------------------------------------------------------------------------------------------------------------- cases

@dataclass
class Case:
    id: str
    algo: str
    kernel: str
    w: tuple                            # match, mismatch, gap (linear) or gapOpen, gapExtend
    band: int = 0
    env: dict = field(default_factory=dict)
    storage: str = "mat"                # a key of FLAGS
    mode: tuple = ()                    # ("zext" | "subst" | "zsub" | "bdx" | "bd2" | "table", ...): the setters behind the creation
    walks: tuple = ("default",)
    texts: object = standard_texts
    texts_args: tuple = ()
    every: int = 1                      # planes are read of every `every`-th pair
    layouts: tuple = layouts.LAYOUTS
    describe: dict = field(default_factory=dict)
    sibling: str = ""                   # a score-only case: the storing case whose texts, oracle and want() it shares

    @property
    def dirs(self):
        return self.storage not in ("mat", "score")

    @property
    def table(self):
        """ANW / ASW / ASG under dpx_batch_set_score_table (score-only) or dpx_batch_set_direction_table (directions)"""
        return bool(self.mode) and self.mode[0] == "table"

    @property
    def scan(self):
        """the fill writes extension records"""
        return bool(self.mode) and self.mode[0] in ("zext", "zsub", "bdx", "bd2") and self.algo == "BAXT"

    @property
    def weights4(self):
        return tuple(self.w) + (-1,) * (4 - len(self.w))


BOTH = ("default", "0")


def _cases():
    out = []
    add = lambda *a, **kw: out.append(Case(*a, **kw))
    lanes = dict(texts=ragged40_texts, every=5)
    for algo in ("LSW", "LNW"):
        add(f"{algo}-k_linear_fill-R2", algo, "k_linear_fill", LIN, env={"DPX_SPLIT": "0", "DPX_LANES": "0", "DPX_R": "2"}, walks=BOTH)
        add(f"{algo}-k_linear_split", algo, "k_linear_split", LIN, env={"DPX_SPLIT": "1"}, walks=BOTH, texts=split_texts)
        add(f"{algo}-k_linear_lanes_pk-ragged40", algo, "k_linear_lanes_pk", LIN, env={"DPX_LANES": "1"}, walks=BOTH, **lanes)
        add(f"{algo}-k_linear_lanes-ragged40", algo, "k_linear_lanes", LIN, env={"DPX_LANES": "1", "DPX_LANES_PK": "0"}, walks=BOTH, **lanes)
        add(f"{algo}-k_linear_fill_pk-coupled", algo, "k_linear_fill_pk", LIN, env={"DPX_PACKED": "1"}, walks=BOTH, texts=coupled_texts)
        add(f"{algo}-k_linear_dir", algo, "k_linear_dir", LIN, storage="dirs", describe={"dir_edges": "lds"})
    for algo, kernel in (("ANW", "k_affine"), ("ASW", "k_asw"), ("ASG", "k_asg")):
        add(f"{algo}-{kernel}_fill-R2", algo, f"{kernel}_fill", AFF, env={"DPX_LANES": "0", "DPX_R": "2"}, walks=BOTH)
        add(f"{algo}-{kernel}_lanes-ragged40", algo, f"{kernel}_lanes", AFF, env={"DPX_LANES": "1"}, walks=BOTH, **lanes)
        add(f"{algo}-{kernel}_dir", algo, f"{kernel}_dir", AFF, storage="dirs", describe={"dir_edges": "lds"})
    for algo, kernel, w, nedges in (("LSW", "k_linear_dir", LIN, 1), ("LNW", "k_linear_dir", LIN, 1), ("ANW", "k_affine_dir", AFF, 2),
                                    ("ASW", "k_asw_dir", AFF, 2), ("ASG", "k_asg_dir", AFF, 2)):
        # the edge rows and the staged reference no longer fit LDS: another load path
        add(f"{algo}-{kernel}-global-edges", algo, kernel, w, storage="dirs", describe={"dir_edges": "global"}, texts=global_edge_texts,
            texts_args=(nedges,), layouts=("canonical", "residues", "embedded"))
    for band in BANDS:
        add(f"BSW-k_banded_fill-B{band}", "BSW", "k_banded_fill", LIN, band=band, env={"DPX_PACKED": "0"}, walks=BOTH)
        add(f"BSW-k_banded_fill_pk-B{band}-couples40", "BSW", "k_banded_fill_pk", LIN, band=band, env={"DPX_PACKED": "1"}, walks=BOTH,
            texts=ragged_couples_texts, every=5)
        add(f"BASW-k_basw_fill-B{band}", "BASW", "k_basw_fill", AFF, band=band, walks=BOTH)
        add(f"BANW-k_banw_fill-B{band}", "BANW", "k_banw_fill", AFF, band=band, walks=BOTH)
        add(f"BAXT-k_baxt_fill-B{band}", "BAXT", "k_baxt_fill", HARSH, band=band, walks=BOTH)
        add(f"BAXT-k_zext_fill-B{band}", "BAXT", "k_zext_fill", HARSH, band=band, mode=("zext", Z, E), walks=BOTH)
        sub = "BANW" if band == 17 else "BAXT"
        add(f"{sub}-k_subst_fill-B{band}", sub, "k_subst_fill", (1, -1) + GAPS, band=band, mode=("subst",), walks=BOTH)
        add(f"BAXT-k_zsub_fill-B{band}", "BAXT", "k_zsub_fill", (1, -1) + GAPS, band=band, mode=("zsub", Z, E), walks=BOTH)
        for algo in ("BANW", "BAXT"):
            add(f"{algo}-k_bdir_fill-B{band}", algo, "k_bdir_fill", HARSH, band=band, storage="bdirs")
        add(f"BANW-k_bdx_fill-B{band}", "BANW", "k_bdx_fill", MM + GAPS, band=band, storage="bdirs", mode=("bdx", -1, -1, True))
        add(f"BAXT-k_bdx_fill-B{band}", "BAXT", "k_bdx_fill", MM + GAPS, band=band, storage="bdirs", mode=("bdx", Z, E, band == 17))
        add(f"BANW-k_bd2_fill-B{band}", "BANW", "k_bd2_fill", (2, -4) + P1, band=band, storage="two", mode=("bd2", -1, -1, False))
        add(f"BAXT-k_bd2_fill-B{band}", "BAXT", "k_bd2_fill", (2, -4) + P1, band=band, storage="two", mode=("bd2", Z, E, True))
        for algo in ("BSW", "BASW"):
            add(f"{algo}-k_bdl_fill-B{band}", algo, "k_bdl_fill", bdl_ref.weights(CODE_OF[algo], AFF), band=band, storage="local")
    # DPX_SCORE_ONLY: every route such a batch can take (the planner never packs or splits it), on the texts and the oracle of its storing
    # sibling; the STORE = false instantiations stage, step and fold differently (tests/test_gpu_score_only.py)
    by_id = {c.id: c for c in out}
    score = lambda sib, R: out.append(replace(by_id[sib], id=sib + "-score-only", storage="score", walks=("default",), sibling=sib,
                                              describe={"store": 0, "rows_per_lane": R}))
    for algo in ("LSW", "LNW"):
        score(f"{algo}-k_linear_fill-R2", 2)
        score(f"{algo}-k_linear_lanes-ragged40", 8)
    for algo, kernel in (("ANW", "k_affine"), ("ASW", "k_asw"), ("ASG", "k_asg")):
        score(f"{algo}-{kernel}_fill-R2", 2)
        score(f"{algo}-{kernel}_lanes-ragged40", 8)
    for band, cpl in zip(BANDS, (1, 4)):
        for sib in ("BSW-k_banded_fill", "BASW-k_basw_fill", "BANW-k_banw_fill", "BAXT-k_baxt_fill", "BAXT-k_zext_fill",
                    ("BANW" if band == 17 else "BAXT") + "-k_subst_fill", "BAXT-k_zsub_fill"):
            score(f"{sib}-B{band}", cpl)
    # the table twins of ANW / ASW / ASG (k_dirtab_* and k_scoretab_*): they launch under the kernel= names of the plain batches.  The table
    # is asymmetric and its map folds every byte outside ACGT onto N, so the fillers and flanks of the layouts are legal and score like
    # sequence.  A score-only case shares the want() of the direction case over the same texts
    tab = dict(mode=("table",))
    for algo, kernel in (("ANW", "k_affine"), ("ASW", "k_asw"), ("ASG", "k_asg")):
        add(f"{algo}-{kernel}_dir-table", algo, f"{kernel}_dir", (1, -1) + GAPS, storage="dirs", describe={"dir_edges": "lds", "subst": 5}, **tab)
        add(f"{algo}-{kernel}_dir-global-edges-table", algo, f"{kernel}_dir", (1, -1) + GAPS, storage="dirs", describe={"dir_edges": "global", "subst": 5},
            texts=global_edge_texts, texts_args=(2,), layouts=("canonical", "residues", "embedded"), **tab)
        add(f"{algo}-{kernel}_fill-R2-score-table", algo, f"{kernel}_fill", (1, -1) + GAPS, env={"DPX_LANES": "0", "DPX_R": "2"}, storage="score",
            describe={"store": 0, "rows_per_lane": 2, "subst": 5}, sibling=f"{algo}-{kernel}_dir-table", **tab)
        add(f"{algo}-{kernel}_lanes-ragged40-score-table", algo, f"{kernel}_lanes", (1, -1) + GAPS, env={"DPX_LANES": "1"}, storage="score",
            describe={"store": 0, "rows_per_lane": 8, "subst": 5}, texts=ragged40_acgt_texts, every=5, **tab)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def plan_case(case):
    """the case as tests/plan_cases.tool_input takes it; plan_tool_input() adds the second gap piece"""
    out = {"name": case.id, "algo": case.algo, "weights": list(case.weights4), "band": case.band, "flags": FLAGS[case.storage], "env": dict(case.env)}
    kind = case.mode[0] if case.mode else None
    if kind == "zext":
        out["mode"] = [case.mode[1], case.mode[2], 0]
    elif kind in ("subst", "table"):
        out["mode"] = [-1, -1, 5]
    elif kind == "zsub":
        out["mode"] = [case.mode[1], case.mode[2], 5]
    elif kind in ("bdx", "bd2"):
        out["mode"] = [case.mode[1], case.mode[2], 5 if case.mode[3] else 0]
    return out


def plan_tool_input(case, laid, first_pair=None, walk="default"):
    import plan_cases

    pc = plan_case(case)
    if walk != "default":
        pc["env"]["DPX_TB_WALK"] = walk
    pc["first_pair"] = laid.first_pair if first_pair is None else first_pair
    whole = layouts.SynthBatch(laid.sequences, laid.pairs[:laid.first_pair + laid.num_pairs], 0, 0)   # plan_tool reads firstPair + numPairs lines
    text = plan_cases.tool_input(pc, whole)
    if case.storage == "two":
        head, sep, table = text.partition("\n" + " ".join(str(int(x)) for x in whole.pairs[0]) + "\n")
        assert sep, "the pair table starts behind the header"
        text = head + "\ngap2 %d %d" % P2 + sep + table
    return text


# ----------------------------------------------------------------------------------------------------------------------- oracles

def build_oracles(d):
    return {"ASW": asw_ref.build(d), "ASG": asg_ref.build(d), "BASW": basw_ref.build(d), "BANW": banw_ref.build(d), "BAXT": baxt_ref.build(d),
            "ZEXT": zext_ref.build(d), "SUBST": subst_ref.build(d), "ZSUB": zsub_ref.build(d), "BD2": bd2_ref.build(d), "BDL": bdl_ref.build(d),
            "DIRTAB": dirtab_ref.build(d)}


def expect(orc, case, ref, qry):
    """what the batch of `case` reports for one pair, in the form test_gpu_poison._read_and_compare takes: score, end, planes (matrix
    batches: int32 arrays) or dirs (direction batches: uint8 arrays; `planes` then only counts them), lines, rec"""
    kind = case.mode[0] if case.mode else None
    ext = case.algo == "BAXT"
    if kind == "table":   # score-only and direction batches alike: the comparators take what their storage reports
        r = orc["DIRTAB"].align(case.algo, ref, qry, TABLE, CODE, *case.w[2:])
        dirs = [r["dirH"], r["dirI"], r["dirD"]]
        return {"score": r["score"], "end": tuple(r["end"]), "planes": dirs, "dirs": dirs, "lines": tuple(r["lines"])}
    if case.storage == "score":   # the oracle of the storing sibling: same algorithm, weights, band and mode
        return expect(orc, BY_ID[case.sibling], ref, qry)
    if case.storage in ("mat", "dirs") and kind in (None, "zext"):
        return _expect(orc, case.algo, ref, qry, case.w, case.band, tuple(case.mode[1:]) if kind else None)
    if kind == "subst":
        r = orc["SUBST"].align(ref, qry, TABLE, CODE, *case.w[2:], case.band, ext)
        return {"score": r["score"], "end": r["end"], "planes": [r["H"], r["I"], r["D"]], "lines": r["lines"]}
    if kind == "zsub":
        r = orc["ZSUB"].align(ref, qry, TABLE, CODE, *case.w[2:], case.band, case.mode[1], case.mode[2])
        return {"score": r["score"], "end": r["end"], "planes": [r["H"], r["I"], r["D"]], "lines": r["lines"], "rec": r["rec"]}
    if case.storage == "local":
        r = orc["BDL"].align(CODE_OF[case.algo], ref, qry, case.w, case.band, planes=True)
        dirs = [r["dirH"], r["dirI"], r["dirD"]][:3 if case.algo == "BASW" else 1]
    elif kind is None:   # k_bdir_fill
        r = orc[case.algo].align(ref, qry, *case.w, case.band, raw=False)
        dirs = list(want_directions(r, case.band))
    else:
        table = (TABLE, CODE) if case.mode[3] else bdx_ref.byte_table(*case.w[:2], b"ACGT")
        if kind == "bdx":
            r = bdx_ref.expect(orc["ZSUB"], ref, qry, *table, *case.w[2:], case.band, ext, case.mode[1], case.mode[2])
        else:
            r = orc["BD2"].expect(ref, qry, *table, case.w[2:], P2, case.band, ext, case.mode[1], case.mode[2])
        dirs = list(r["dirs"])
    return {"score": r["score"], "end": tuple(r["end"]), "planes": dirs, "dirs": dirs, "lines": tuple(r["lines"]), "rec": r.get("rec")}


_WANT = {}


def want(orc, case):
    """the oracle's results of a case's texts, computed once and shared by every layout and walk, and by a score-only case and its
    sibling; nothing modifies them"""
    key = want_key(case)
    if key not in _WANT:
        _WANT[key] = [expect(orc, case, ref, qry) for ref, qry in texts_of(case)]
    return _WANT[key]


def want_key(case):
    return case.sibling or case.id


def configure(case, b):
    """the setters of `case` on the fresh batch `b`"""
    kind = case.mode[0] if case.mode else None
    if kind == "zext":
        b.set_extension(*case.mode[1:])
    elif kind == "subst":
        b.set_substitution(TABLE, CODE)
    elif kind == "zsub":
        b.set_extension_table(case.mode[1], case.mode[2], TABLE, CODE)
    elif kind == "bd2":
        b.set_second_gap(*P2)
    elif kind == "table":
        (b.set_score_table if case.storage == "score" else b.set_direction_table)(TABLE, CODE)
    if kind in ("bdx", "bd2") and (case.mode[1] >= 0 or case.mode[2] >= 0 or case.mode[3]):
        b.set_direction_scoring(case.mode[1], case.mode[2], *((TABLE, CODE) if case.mode[3] else (None, None)))
