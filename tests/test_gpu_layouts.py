"""Every fill kernel, walk and export under every sequence-buffer layout of tests/layouts.py, against the CPU oracle of its algorithm.

The C ABI lets a batch's strings sit anywhere in the flat buffer -- any order, any residue, touching, overlapping, shared, behind
kilobytes that belong to other batches -- and the engine has code that depends on exactly that: stage_bytes / load4 / CharWin /
load_query_rows read aligned blocks AROUND a string, the planner's LDS budgets assume the worst residue, sequence_window uploads
[smallest offset, largest end) only and rebases every index, dpx_batch_set_reversed builds its copies on the rebased table.  Every other
test feeds all of it synth's one layout (ascending, reference first, a NUL on both sides of every string, the window at byte 0).

tests/layout_cases.py has one small batch per kernel of dpx_route_kernel_name (27), forced as the kernel's own test forces it and
asserted from dpx_batch_describe; each runs under all six layouts (the direction kernels' global-edge-row variants under three), with
both walks where DPX_TB_WALK chooses one, and everything the batch reports -- results, extension records, every plane of every pair (of
every fifth pair in the 40-pair batches of the kernels that pack several pairs into a wave), every traceback, the text and its offsets,
the CIGAR records and ops under both flags -- must equal the oracle bit for bit.  The oracle's answer depends on the texts alone and is
computed once per case; no GPU batch is compared with another.  The DPX_SCORE_ONLY cases (every route such a batch can take) share the
want() of their storing siblings and go through tests/test_gpu_score_only.py's comparator; the table twins of ANW / ASW / ASG run an
asymmetric five-letter table whose map folds the layouts' fillers and flanks onto N.  tests/test_layouts.py shows on the oracle alone that the `embedded`
layout is not vacuous (the flanks change every case's answer) and that the planner decides the same for every layout.

Then dpx_batch_set_reversed on a rebased window and on pairs that share bytes (BANW and BAXT as matrix, band-direction and two-piece
batches, alternating pairs reversed, against the oracle on host-reversed strings by the rules of include/dpx_align.h), and packed2
input cut out of the middle of a buffer and laid out in descending order on a linear, an affine and a band-direction route."""
import numpy as np
import pytest

import layout_cases as L
from layouts import lay
from test_gpu_poison import _read_and_compare
from test_gpu_score_only import _score_only

pytestmark = pytest.mark.gpu

PARAMS = [pytest.param(c, layout, walk, id=f"{c.id}-{layout}-walk_{walk}") for c in L.CASES for layout in c.layouts for walk in c.walks]
REVERSED = [c for c in L.CASES if c.id in ("BANW-k_banw_fill-B17", "BAXT-k_baxt_fill-B17", "BANW-k_bdir_fill-B17", "BAXT-k_bdir_fill-B17",
                                            "BANW-k_bd2_fill-B17", "BAXT-k_bd2_fill-B17")]
PACKED2 = [c for c in L.CASES if c.id in ("LSW-k_linear_fill-R2", "ANW-k_affine_fill-R2", "BAXT-k_bdir_fill-B17")]


@pytest.fixture(scope="module")
def oracles(tmp_path_factory):
    return L.build_oracles(tmp_path_factory.mktemp("layout_oracles"))


def _environment(monkeypatch, case, walk="default"):
    for k in L.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if walk != "default":
        monkeypatch.setenv("DPX_TB_WALK", walk)


def _ran(case, d, walk="default"):
    assert d["algo"] == case.algo and d["kernel"] == case.kernel, d
    assert all(d.get(k) == v for k, v in case.describe.items()), d
    if case.storage == "score":
        assert d["store"] == 0 and (d["waves"] > 0) == case.kernel.endswith("_lanes"), d
    if "traceback" in d and case.walks == L.BOTH:
        assert d["traceback"].endswith("_wave") == (walk == "default"), d


@pytest.mark.parametrize("case,layout,walk", PARAMS)
def test_every_kernel_under_every_layout(gpu, oracles, monkeypatch, case, layout, walk):
    _environment(monkeypatch, case, walk)
    texts = L.texts_of(case)
    laid = lay(layout, texts)
    want = L.want(oracles, case)
    with gpu.Batch(L.CODE_OF[case.algo], laid.sequences, laid.pairs, *case.w, band=case.band, flags=L.FLAGS[case.storage], **laid.kwargs) as b:
        L.configure(case, b)
        d = b.describe()
        _ran(case, d, walk)
        assert d["seq_input"] == "bytes" and b.num_pairs == len(texts)
        b.fill()
        if case.storage == "score":
            _score_only(b, want, (case.id, layout))
        else:
            _read_and_compare(gpu, b, want, case.dirs, True if case.scan else None, (case.id, layout, walk), picks=range(0, len(texts), case.every))


SCORE_ONLY_ROUTES = {"k_linear_fill", "k_linear_lanes", "k_affine_fill", "k_asw_fill", "k_asg_fill", "k_affine_lanes", "k_asw_lanes", "k_asg_lanes",
                     "k_banded_fill", "k_basw_fill", "k_banw_fill", "k_baxt_fill", "k_zext_fill", "k_subst_fill", "k_zsub_fill"}
SCORE_TABLE_ROUTES = {"k_affine_fill", "k_asw_fill", "k_asg_fill", "k_affine_lanes", "k_asw_lanes", "k_asg_lanes"}
DIRECTION_TABLE_ROUTES = {"k_affine_dir", "k_asw_dir", "k_asg_dir"}


def test_what_the_table_above_exercised():
    """all 27 fill kernels, both walks where there is a choice, the reversed setter in three storage modes and packed2 on three routes,
    each under layouts other than the canonical one; every (kernel, storage, table or not) combination -- the score-only routes and the
    table twins launch under the storing kernels' names -- under at least `residues` and `embedded`"""
    ran, combos = {}, {}
    for p in PARAMS:
        case, layout, walk = p.values
        ran.setdefault(case.kernel, set()).add((layout, walk))
        combos.setdefault((case.kernel, case.storage, case.table), set()).add(layout)
    for combo, seen in combos.items():
        assert {"residues", "embedded"} <= seen, combo
    assert {k for k, storage, table in combos if storage == "score" and not table} == SCORE_ONLY_ROUTES
    assert {k for k, storage, table in combos if storage == "score" and table} == SCORE_TABLE_ROUTES
    assert {k for k, storage, table in combos if storage == "dirs" and table} == DIRECTION_TABLE_ROUTES
    assert {c.band for c in L.CASES if c.storage == "score" and c.band} == set(L.BANDS)
    for kernel in DIRECTION_TABLE_ROUTES:   # the global edge rows under the table too, under the three layouts of the plain ones
        assert any(c.kernel == kernel and c.table and c.describe["dir_edges"] == "global" and c.layouts == ("canonical", "residues", "embedded") for c in L.CASES)
    assert set(ran) == L.KERNELS and len(ran) == 27
    for kernel, seen in ran.items():
        assert {"residues", "embedded"} <= {layout for layout, _ in seen}, kernel
        if any(c.kernel == kernel and c.walks == L.BOTH for c in L.CASES):
            assert {w for layout, w in seen if layout != "canonical"} == {"default", "0"}, kernel
    full = [c for c in L.CASES if set(c.layouts) == set(L.layouts.LAYOUTS)]
    assert {c.kernel for c in full} == L.KERNELS                      # (the three-layout cases are extra: the global edge rows)
    assert {(c.algo, c.storage) for c in REVERSED} == {(a, s) for a in ("BANW", "BAXT") for s in ("mat", "bdirs", "two")}
    assert {c.kernel for c in PACKED2} == {"k_linear_fill", "k_affine_fill", "k_bdir_fill"}


# ------------------------------------------------------------------------------------------------------------------- reversed pairs

def _reversed_want(oracles, case, texts, mask):
    """the oracle on host-reversed strings for the masked pairs: results, records and planes stay in that frame, the lines come back to
    front and the alignment coordinates count from the other end (include/dpx_align.h, dpx_batch_set_reversed)"""
    plain, out = L.want(oracles, case), []
    for p, (ref, qry) in enumerate(texts):
        if not mask[p]:
            out.append(plain[p])
            continue
        r = dict(L.expect(oracles, case, ref[::-1], qry[::-1]))
        on_ref = sum(1 for c in r["lines"][0] if c != ord("_"))
        on_qry = sum(1 for c in r["lines"][2] if c != ord("_"))
        r["lines"] = tuple(x[::-1] for x in r["lines"])
        r["cigar_end"] = (len(qry) - r["end"][0] + on_qry, len(ref) - r["end"][1] + on_ref)
        out.append(r)
    return out


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("layout", ["windowed", "shared"])
@pytest.mark.parametrize("case", REVERSED, ids=lambda c: c.id)
def test_reversed_pairs_on_a_rebased_window_and_on_shared_bytes(gpu, oracles, monkeypatch, case, layout, first):
    """the setter's copies are built on the rebased table: here the window starts at byte 4101 (`windowed`), and a pair's reference and
    query are the same bytes or overlap, and masked and unmasked pairs share one reference (`shared`)"""
    _environment(monkeypatch, case)
    texts = L.texts_of(case)
    laid = lay(layout, texts)
    mask = (np.arange(len(texts)) % 2 == first).astype(np.uint8)
    want = _reversed_want(oracles, case, texts, mask)
    assert any(w["lines"] != p["lines"] for w, p in zip(want, L.want(oracles, case)))
    with gpu.Batch(L.CODE_OF[case.algo], laid.sequences, laid.pairs, *case.w, band=case.band, flags=L.FLAGS[case.storage], **laid.kwargs) as b:
        if first:   # either call order
            b.set_reversed(mask)
            L.configure(case, b)
        else:
            L.configure(case, b)
            b.set_reversed(mask)
        d = b.describe()
        _ran(case, d)
        assert d["reversed"] == int(mask.sum()), d
        b.fill()
        _read_and_compare(gpu, b, want, case.dirs, True if case.scan else None, (case.id, layout, "reversed", first))


# ------------------------------------------------------------------------------------------------------------------- packed2

@pytest.mark.parametrize("layout", ["windowed", "tight_reversed"])
@pytest.mark.parametrize("case", PACKED2, ids=lambda c: c.id)
def test_packed2_input_under_layouts(gpu, oracles, monkeypatch, case, layout):
    """2-bit input: the device expands from the 16-base boundary below the window, so the residues are the host's"""
    _environment(monkeypatch, case)
    texts = L.texts_of(case)
    laid = lay(layout, texts)
    pk, al = gpu.pack2(laid.sequences, laid.pairs)
    with gpu.Batch(L.CODE_OF[case.algo], None, laid.pairs, *case.w, band=case.band, flags=L.FLAGS[case.storage], packed2=(pk, al, laid.sequences.size),
                   **laid.kwargs) as b:
        L.configure(case, b)
        d = b.describe()
        _ran(case, d)
        assert d["seq_input"] == "packed2", d
        b.fill()
        _read_and_compare(gpu, b, L.want(oracles, case), case.dirs, True if case.scan else None, (case.id, layout, "packed2"))
