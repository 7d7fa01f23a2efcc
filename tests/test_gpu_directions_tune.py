"""DPX_KEEP_DIRECTIONS together with DPX_TUNE_PLACEMENT: a directions batch whose code pool passes 1 GiB is shopped for with its own fill
on several candidate pools; the fills, the kept pool and everything read back afterwards must follow the pool the batch ends up with."""
import numpy as np
import pytest

import oracle_py as O

from dpx_gpu_genomics_project_amd.synth import make_batch

pytestmark = pytest.mark.gpu


def test_tuned_directions_batch_matches_matrices_batch(gpu):
    sb = make_batch(2000, 1024, 1024, seed=17)
    with gpu.Batch(gpu.ALGO_LSW, sb.sequences, sb.pairs, 3, -1, -2, flags=gpu.KEEP_DIRECTIONS | gpu.TUNE_PLACEMENT) as db:
        d = db.describe()
        assert db.info()["matrix_bytes"] >= 1 << 30
        assert len(str(d["pool_fill_ms"]).split(",")) >= 2, d  # the pool was shopped for with the batch's fill
        db.fill()
        got = db.results()
        db.output_begin(0)
        dtext, doff = db.output_end()
        dlines = [db.traceback(p) for p in (0, 999, 1999)]
        ddir = db.directions(1999)
    with gpu.Batch(gpu.ALGO_LSW, sb.sequences, sb.pairs, 3, -1, -2) as mb:
        mb.fill()
        want = mb.results()
        mb.output_begin(0)
        mtext, moff = mb.output_end()
        mlines = [mb.traceback(p) for p in (0, 999, 1999)]
        H = mb.matrix(1999).astype(np.int32)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    assert dtext == mtext and np.array_equal(doff, moff)
    assert dlines == mlines
    r = O.lsw(sb.ref(1999), sb.qry(1999), 3, -1, -2)  # the exported codes come from the kept pool
    assert np.array_equal(ddir, r.dir)
    assert np.array_equal(H, r.H)
