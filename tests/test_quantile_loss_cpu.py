"""CPU tests of ``ops.quantile_huber_loss``: the fp32 torch fallback
against the float64 reference under the derived bound ``(M + 16) 2^-24
S`` (``util_quantile_loss.reference64``), argument validation and the
``RAINBOW(distribution="quantile")`` option.
"""
import numpy as np
import pytest
import torch as t

from machin_amd import ops
from machin_amd.frame.algorithms import RAINBOW
from util_quantile_loss import (
    PixelQuantileNet, all_cases, make_case, reference64, run_op,
    seeded_quantile_update, within_bound,
)


@all_cases
def test_fallback_within_the_bound(shape, tie, kappa, given_taus, dtype):
    case = make_case(shape, given_taus, dtype, tie)
    ref, bound = reference64(shape, given_taus, dtype, kappa, tie)
    result = run_op(ops.quantile_huber_loss, case, kappa)
    assert not tie or t.equal(result[2], case.want_best)
    assert within_bound(case, result, ref, bound, "fallback")


@pytest.mark.parametrize("A,N,M,kappa,dtype", [
    (3, 257, 2, 1.0, None), (3, 2, 257, 1.0, None), (65, 2, 2, 1.0, None),
    (3, 2, 2, -1.0, None), (3, 2, 2, float("nan"), None),
    (3, 2, 2, 1.0, t.bfloat16), (3, 2, 2, 1.0, t.float16)])
def test_rejects_violated_limits(A, N, M, kappa, dtype):
    """``dtype``: of ``next_online`` alone (bf16) or of all three."""
    theta, nxt = t.zeros(2, A, N), t.zeros(2, A, M).to(dtype)
    if dtype == t.float16:
        theta = theta.half()
    with pytest.raises(ValueError):
        ops.quantile_huber_loss(theta, t.zeros(2).long(), nxt, t.zeros(
            2, A, M).to(theta.dtype), t.zeros(2), t.zeros(2), 0.5, kappa)


def test_rainbow_update_moves_the_parameters():
    algo, before, loss = seeded_quantile_update()
    assert algo.fused_loss and "quantile_huber_loss" in ops.__all__
    assert np.isfinite(loss) and loss > 0
    assert all(not t.equal(p, p0)
               for p, p0 in zip(algo.qnet.parameters(), before))
    values = t.arange(24.0).view(1, 3, 8)
    assert t.equal(algo._q_values(values), values.mean(dim=2))


def test_rainbow_rejects_logits_and_takes_config_keys():
    nets = PixelQuantileNet(), PixelQuantileNet()
    for options in (dict(distribution="quantile", dist_from_logits=True),
                    dict(distribution="iqn")):
        with pytest.raises(ValueError):
            RAINBOW(*nets, t.optim.Adam, -1.0, 1.0, **options)
    config = RAINBOW.generate_config({})
    config["frame_config"].update(
        models=[PixelQuantileNet] * 2, distribution="quantile",
        huber_kappa=0.25)
    algo = RAINBOW.init_from_config(config)
    assert algo.distribution == "quantile" and algo.huber_kappa == 0.25
