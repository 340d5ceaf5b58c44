"""The predictors' host layer without a GPU: one parse of the head layout answers which evaluation takes the heads (the answers
are pinned to what the two separate parses gave before they were merged), per-run state is declared by ``__init__``, and one
dict holds every derived constant."""
import itertools

import pytest
import torch

FLAGS = list(itertools.product((False, True), repeat=3))            # (ln, tailact, twolayerlin), twolayerlin fastest
# Recorded from the commit BEFORE the single parse, per (predictor, H), one digit per entry of FLAGS:
# 4 = the module conditions of `_heads_grouped` held, 2 = `_heads_plan(H) is not None`, 1 = `_fused_plan(H) is not None`.
# All 160 combinations were recorded; the four predictors gave the same rows (they share the constructor of the heads).
RECORDED = {32: "66666666", 64: "66666666", 96: "00000000", 128: "76767676", 256: "76767676"}
PREDICTORS = ("cn5", "cn7", "cn8", "cn6")


def _grouped_conditions(pred, H):
    """The conditions on the modules under which the layer-by-layer evaluation ran without a class order, restated."""
    from ocn_amd import ops
    from ocn_amd.model import _stages
    if H not in ops.LINEAR_WIDTHS or not ops.fast_linear:
        return False
    sa, sb, sx = _stages(pred.xcn1lin, H), _stages(pred.xcn2lin, H), _stages(pred.xijlin, H)
    if sa is None or sb is None or sx is None or len(sa) != 3 or len(sb) != 3 or len(sx) not in (1, 2):
        return False
    return sa[2][1] is None and not sa[2][2] and sb[2][1] is None and not sb[2][2]


def _code(pred, H):
    return 4 * int(pred._layout(H).layered) + 2 * int(pred._heads_plan(H) is not None) + int(pred._fused_plan(H) is not None)


@pytest.mark.parametrize("H", sorted(RECORDED))
@pytest.mark.parametrize("name", PREDICTORS)
def test_head_plans_answer_as_the_separate_parses_did(name, H):
    from ocn_amd.model import predictor_dict
    got = ""
    for ln, tailact, two in FLAGS:
        pred = predictor_dict[name](H, H, 1, 2, 0.0, ln=ln, tailact=tailact, twolayerlin=two).eval()
        assert pred._layout(H).layered == _grouped_conditions(pred, H), (ln, tailact, two)
        plan, fplan = pred._heads_plan(H), pred._fused_plan(H)
        assert plan is None or (len(plan) == 3 and len(plan[0]) == len(plan[1]) == 3 and len(plan[2]) == (1 if tailact else 2))
        assert fplan is None or (len(fplan) == 5 and fplan[4] is pred.lin[-1] and fplan[3][0] is pred.lin[0])
        got += str(_code(pred, H))
    assert got == RECORDED[H]


def test_head_plans_refuse_a_wider_input():
    """in_channels = 2 H: the first layers are not H x H, no plan applies (recorded: 0)."""
    from ocn_amd.model import predictor_dict
    H = 64
    pred = predictor_dict["cn5"](2 * H, H, 1, 2, 0.0).eval()
    assert not _grouped_conditions(pred, H) and _code(pred, H) == 0


def test_a_lin_without_the_dot_tail_is_layered_but_not_skipping():
    """``lin`` not ending in Linear(H, 1) (recorded: 4 at H = 64 and 128): the layered form without a class order does not
    look at ``lin``, the skipping form needs its tail to scatter the scores, the fused kernel evaluates it."""
    import torch.nn as nn
    from ocn_amd.model import predictor_dict
    for H in (64, 128):
        pred = predictor_dict["cn5"](H, H, 2, 2, 0.0).eval()
        assert isinstance(pred.lin[-1], nn.Linear) and pred.lin[-1].out_features == 2
        lay = pred._layout(H)
        assert _grouped_conditions(pred, H) and _code(pred, H) == 4
        assert (lay.layered, lay.skipping, lay.fused, lay.sl, lay.tail) == (True, False, False, None, None)


def test_the_recorded_examples():
    from ocn_amd.model import predictor_dict
    pred = predictor_dict["cn5"](128, 128, 1, 2, 0.0, twolayerlin=True).eval()
    assert (pred._heads_plan(128) is not None, pred._fused_plan(128) is not None) == (True, False)
    pred = predictor_dict["cn5"](128, 128, 1, 2, 0.0).eval()
    assert (pred._heads_plan(128) is not None, pred._fused_plan(128) is not None) == (True, True)


@pytest.mark.parametrize("name", PREDICTORS)
def test_per_run_state_is_declared_and_one_dict_holds_the_caches(name):
    from ocn_amd.model import predictor_dict
    pred = predictor_dict[name](32, 32, 1, 2, 0.0)
    state = vars(pred)
    assert state["_skip_state"] is None and state["_rowsum_cache"] is None and state["_ws_slots"] == [] and state["_cache"] == {}
    before = set(state)
    pred.eval()
    assert pred._heads_plan(32) is not None and pred._mix_coef().shape == (3,)
    assert set(pred._cache) == {"layout", "coef"}
    assert set(vars(pred)) == before                               # nothing appears beside the declared attributes
    pred.train()
    pred.eval()
    assert pred._cache == {}
    coef = pred._mix_coef()
    with torch.no_grad():
        pred.alpha.add_(1.0)                                       # an in-place edit moves the version counter: recomputed
    assert not torch.equal(pred._mix_coef(), coef)
    pred.float()                                                   # _apply: parameters may be re-created
    assert pred._cache == {}
