"""tests/bdx_oracle.c (band-only, rolling anti-diagonals) against tests/zsub_oracle.c (full matrices) on the CPU: the record and the
chosen score and end cell agree on the shared fuzz set and on the drop sweep of tests/test_gpu_bdx.py, in every mode of k_bdx_fill; and
the sweep covers what it is meant to cover: every pair drops, on the anti-diagonal the issue states, and for every cells-per-lane count
the dropping steps reach every residue of a store group."""
import numpy as np
import pytest

import bdx_ref
import subst_ref
import zsub_ref

TABLE, CODE = zsub_ref.acgtn_table()


@pytest.fixture(scope="module")
def oracles(tmp_path_factory):
    d = tmp_path_factory.mktemp("bdx_oracle")
    return bdx_ref.build(d), zsub_ref.build(d)


def _same(bo, zs, ref, qry, table, code, gaps, band, ext, z, e):
    got = bo.fill(ref, qry, table, code, *gaps, band, ext=ext, zdrop=z, end_bonus=e)
    want = bdx_ref.expect(zs, ref, qry, table, code, *gaps, band, ext=ext, zdrop=z, end_bonus=e)
    assert (got["score"], got["end"]) == (want["score"], want["end"]), (ref, qry, band, ext, z, e)
    if want["rec"] is not None:
        assert got["rec"] == want["rec"], (ref, qry, band, z, e)
    return got


@pytest.mark.parametrize("mode", bdx_ref.MODES, ids=[m[0] for m in bdx_ref.MODES])
def test_fuzz(oracles, mode):
    bo, zs = oracles
    _, algo, with_table, drop, bonus = mode
    code = subst_ref.fuzz_code()
    seen = 0
    for band, texts in zsub_ref.fuzz_texts().items():
        for table in zsub_ref.FUZZ_TABLES:
            if not with_table and table[0][1] != table[1][0]:
                continue  # (not a match / mismatch pair)
            for z in (zsub_ref.FUZZ_Z if drop else (-1,)):
                for ref, qry in texts:
                    if algo == bdx_ref.BANW and abs(len(ref) - len(qry)) >= band:
                        continue
                    _same(bo, zs, ref, qry, np.array(table, np.int8), code, zsub_ref.FUZZ_GAPS, band, algo == bdx_ref.BAXT, z,
                          zsub_ref.FUZZ_E if bonus else -1)
                    seen += 1
    assert seen >= 100


@pytest.mark.parametrize("band", sorted(bdx_ref.SWEEP_BANDS))
def test_sweep_drops_where_stated(oracles, band):
    bo, zs = oracles
    for L, ref, qry in bdx_ref.sweep_cases(band):
        for z in bdx_ref.SWEEP_Z:
            got = _same(bo, zs, ref, qry, TABLE, CODE, bdx_ref.SWEEP_GAPS, band, True, z, bdx_ref.SWEEP_E)
            assert got["rec"]["flags"] & 1, (band, L, z)
            assert got["rec"]["lastDiag"] == bdx_ref.sweep_last_diag(band, L, z), (band, L, z, got["rec"])
        # the same pairs in every other mode: without the drop test, BANW (the equal lengths admit it), and without a table, that is
        # under the table that scores as byte equality does
        bt, bc = bdx_ref.byte_table(2, -3)
        for ext, z, e, table, code in ((True, -1, bdx_ref.SWEEP_E, TABLE, CODE), (True, -1, -1, TABLE, CODE), (False, -1, -1, TABLE, CODE),
                                       (True, -1, bdx_ref.SWEEP_E, bt, bc), (True, 7, bdx_ref.SWEEP_E, bt, bc), (True, 12, bdx_ref.SWEEP_E, bt, bc)):
            _same(bo, zs, ref, qry, table, code, bdx_ref.SWEEP_GAPS, band, ext, z, e)


def test_sweep_reaches_every_group_residue_and_both_parities(oracles):
    bo, _ = oracles
    residues, parities = {}, {}
    for band in bdx_ref.SWEEP_BANDS:
        c = bdx_ref.cpl(band)
        for L, ref, qry in bdx_ref.sweep_cases(band):
            for z in bdx_ref.SWEEP_Z:
                last = bo.fill(ref, qry, TABLE, CODE, *bdx_ref.SWEEP_GAPS, band, zdrop=z, end_bonus=bdx_ref.SWEEP_E)["rec"]["lastDiag"]
                residues.setdefault(c, set()).add((last - 2) % (32 // c))
                parities.setdefault(c, set()).add(last & 1)
                if band == 16:
                    assert last % 2 == 0, (L, z, last)  # band 16 alone reaches even anti-diagonals only
    for c in (1, 2, 4, 8):
        assert residues[c] == set(range(32 // c)), (c, sorted(residues[c]))
        assert parities[c] == {0, 1}, c


def test_every_c_drops_in_the_interior_phase_on_either_step(oracles):
    """The partial-group store, the break after the first and after the second step of a loop body and the guard on the tail loop are
    reached from the interior loop only when a drop lies in it.  From the kernel's own geometry (bdx_ref.phase_of): the interior pairs
    of every band from 100 on drop there at both Z, those with A / C tails on the first step of a body and those with G / A tails on
    the second; and with the sweep's pairs every cells-per-lane count has an interior drop on either step.  (The sweep alone leaves C = 4 and C = 8 without one: its tails of
    60 bases put those drops into the tail phase, which this test also states.)"""
    bo, zs = oracles
    seen = {}

    def drop(band, ref, qry, z):
        got = _same(bo, zs, ref, qry, TABLE, CODE, bdx_ref.SWEEP_GAPS, band, True, z, bdx_ref.SWEEP_E)
        assert got["rec"]["flags"] & 1, (band, z)
        return bdx_ref.phase_of(len(qry), len(ref), band, got["rec"]["lastDiag"] - 2)

    for band in bdx_ref.SWEEP_BANDS:
        c = bdx_ref.cpl(band)
        for _, ref, qry in bdx_ref.sweep_cases(band):
            for z in bdx_ref.SWEEP_Z:
                phase, step = drop(band, ref, qry, z)
                seen.setdefault((c, phase), set()).add(step)
                if band >= 200:
                    assert phase == "tail", (band, z)
    for band in bdx_ref.INTERIOR_BANDS:
        c = bdx_ref.cpl(band)
        for _, ref, qry, step in bdx_ref.interior_cases(band):
            for z in bdx_ref.SWEEP_Z:
                assert drop(band, ref, qry, z) == ("interior", step), (band, z)
                seen.setdefault((c, "interior"), set()).add(step)
            for ext, zz, e in ((True, -1, bdx_ref.SWEEP_E), (True, -1, -1), (False, -1, -1)):
                _same(bo, zs, ref, qry, TABLE, CODE, bdx_ref.SWEEP_GAPS, band, ext, zz, e)
    for c in (1, 2, 4, 8):
        assert seen.get((c, "interior")) == {0, 1}, (c, seen)
        assert seen.get((c, "tail")) or c == 1, (c, seen)  # ... and a drop in the tail phase at every C the sweep puts one there
