"""What the last call left in the right-hand sides of a handle (csrc/ck_api.hip: AuxState): after the entry points whose rows
are not ck_predict's, ck_verify_model and ck_aux_finish refuse with the sentence that names the call; after ck_loocv
ck_verify_model asks for a ck_predict; after ck_predict it answers as on a fresh handle."""
import numpy as np
import pytest

from tests import dense_chains as dc
from tests.test_gpu_entry_edge_sizes import handle, native   # noqa: F401 (native: the fixture)

pytestmark = pytest.mark.gpu

VERIFY = "ck_verify_model: the last call was {}, {}; call ck_predict with the sites to check first"
FINISH = "ck_aux_finish: the last call was {}; call ck_aux_begin first"


def test_refusals_name_the_last_call(native):
    ds = dc.data_set(dc.SMALL)
    pc = dc.pred_sites(np.random.default_rng(7), ds.metric, 5)
    fresh = handle(native, ds)
    fresh.predict(0, pc)
    want = fresh.verify_model()
    fresh.close()

    h = handle(native, ds)
    h.aux_begin(0, pc)   # (the wrapper's aux_finish sizes its outputs by the last aux_begin)

    def refused(call, clause):
        with pytest.raises(native.NativeError) as e:
            h.verify_model()
        assert str(e.value) == VERIFY.format(call, clause)
        with pytest.raises(native.NativeError) as e:
            h.aux_finish()
        assert str(e.value) == FINISH.format(call)

    h.predict_blocks(0, pc, [0, 1, 0, 1, 1], np.ones(5), 2)
    refused("ck_predict_blocks", "whose right-hand sides are block sums")
    assert h.loglik(True)[0] == 0
    refused("ck_loglik", "whose right-hand sides are the data sites' unit rows")
    for k in range(2):
        h.set_trend(k, dc.design("constant", ds.coords[k], ds.coords[k]))
    h.predict_universal(0, pc, dc.design("constant", ds.coords[0], pc))
    refused("ck_predict_universal", "for which the simple-kriging verdict does not apply")
    assert h.cv_folds(0, np.arange(len(ds.coords[0])) % 2)[0] == 0
    refused("ck_cv_folds", "whose right-hand sides are the withheld data's unit rows")
    h.loocv(0, len(ds.coords[0]))
    with pytest.raises(native.NativeError) as e:
        h.verify_model()
    assert str(e.value) == "ck_verify_model needs the solved right-hand sides of a preceding ck_predict"
    h.predict(0, pc)
    assert h.verify_model() == want
    h.close()


def test_predict_blocks_leaves_the_point_path_timings(native):
    """Slots 0 .. 15 of ck_timings describe the last point-path calls.  ck_predict_blocks -- in one pass, in three passes
    through the assembly stage, and refused -- leaves every one of them as it was, and a ck_predict afterwards returns the first
    one's bits."""
    ds = dc.data_set(dc.SMALL)
    pc = dc.pred_sites(np.random.default_rng(7), ds.metric, 5)
    block, w = [0, 1, 0, 1, 1], np.ones(5)
    h = handle(native, ds)
    pred, err = h.predict(0, pc)
    point = list(h.timings().items())[:16]
    assert [k for k, _ in point][:5] == ["assemble_sigma_ms", "factor_ms", "assemble_aux_ms", "solve_ms", "reduce_ms"]
    assert all(dict(point)[k] > 0.0 for k in ("assemble_sigma_ms", "factor_ms", "assemble_aux_ms", "solve_ms", "reduce_ms"))
    h.set_option("block_chunk", 0)
    h.predict_blocks(0, pc, block, w, 2, want_cov=True)
    assert list(h.timings().items())[:16] == point and h.timings()["blocks_chunks"] == 1
    h.set_option("block_chunk", 2)
    h.predict_blocks(0, pc, block, w, 2, want_cov=True)
    t = h.timings()
    assert list(t.items())[:16] == point and t["blocks_chunks"] == 3 and t["blocks_assemble_ms"] > 0.0
    with pytest.raises(native.NativeError) as e:
        h.predict_blocks(0, pc, [0, 1, 2, 1, 1], w, 2)
    assert str(e.value) == "ck_predict_blocks: block label 2 of site 2 is outside [0, r)"
    assert list(h.timings().items())[:16] == point
    again = h.predict(0, pc)
    assert np.array_equal(again[0], pred) and np.array_equal(again[1], err)
    h.close()
