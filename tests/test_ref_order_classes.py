"""CPU tier of the rank-class table (common.RANK_CLASS_TABLE) that tests/test_gpu_ref_order_edges.py runs on the GPU: the oracle's target
mode still puts every row in its classes, the table covers every class, and the float64 rank formula (common.rank_formula) reproduces
the oracle's n, cov and -ll on every row."""
import numpy as np
import pytest

import common as cm


@pytest.mark.parametrize("row", cm.RANK_CLASS_TABLE, ids=lambda r: "s%d_%dx%d_ty%g_i%g_d%g" % r[:6])
def test_each_row_is_in_its_rank_classes(row):
    o, o_no_q3 = cm.rank_class_row_oracle(row)
    assert o["n"] == row[6]
    assert cm.rank_classes(o["residuals"], o_no_q3["residuals"], o["n_selected"]) == set(row[7])
    f = cm.rank_formula(o["residuals"], None, True)
    assert f["n"] == o["n"] and f["kept"] == o["n"] // 50 * 50
    if o["n"] >= 6:
        scale = np.sqrt(np.abs([o["cov"][0] ** 2, o["cov"][0] * o["cov"][2], o["cov"][2] ** 2]))
        assert (np.abs(f["cov"] - o["cov"]) <= 1e-7 * scale).all()           # (the oracle's cov is rounded to float32)
        assert abs(f["neg_ll"] - o["neg_ll"]) <= 1e-6 * abs(o["neg_ll"])    # (the oracle's -ll is a float)
    else:
        assert f["neg_ll"] is None


def test_the_table_covers_every_rank_class():
    seen = set()
    for row in cm.RANK_CLASS_TABLE:
        seen |= set(row[7])
    assert seen == set(cm.RANK_CLASSES)


def test_rank_formula_weighted_pass_against_the_oracle():
    """the weighted pass of the formula (float32 weights 7 / (5 + r^T P_prev r)) against the oracle's target mode on the rows with a
    log-likelihood: the oracle's residual plane, its first-pass precision"""
    import oracle.pyoracle as po
    for row in cm.RANK_CLASS_TABLE:
        if row[6] < 6:
            continue
        seed, w, h, ty, ithr, dthr = row[:6]
        ref, cur = cm.oracle_pyramids(cm.synth(seed, w, h), 1)
        T34 = po.se3_exp(np.array([0.0, ty, 0.0, 0.0, 0.0, 0.0]))[:3]
        mode = po.QUIRKS | po.Q_DROP_ODD | po.Q_LOGLIK_TAIL | po.X_PAIRING_F64
        o1 = po.level_iteration(ref, cur, 0, T34, first=True, mode=mode, ithr=ithr, dthr=dthr)
        o2 = po.level_iteration(ref, cur, 0, T34, P_prev=o1["P"], first=False, mode=mode, ithr=ithr, dthr=dthr, want_residuals=True)
        f = cm.rank_formula(o2["residuals"], o1["P"], False)
        scale = np.sqrt(np.abs([o2["cov"][0] ** 2, o2["cov"][0] * o2["cov"][2], o2["cov"][2] ** 2]))
        assert f["n"] == o2["n"]
        assert (np.abs(f["cov"] - o2["cov"]) <= 1e-7 * scale).all(), row
        assert abs(f["neg_ll"] - o2["neg_ll"]) <= 1e-6 * abs(o2["neg_ll"]), row
