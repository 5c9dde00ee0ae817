"""GPU tests of the fused quantile-regression loss head against the
float64 reference of ``util_quantile_loss`` on dyadic inputs, and
``RAINBOW(distribution="quantile")`` on ``cuda:0``.

Bound (``reference64``): ``(M + 16) 2^-24`` times the magnitude sums; a
bf16 gradient adds ``2^-8 |ref|``; ``best``, ``target`` and untaken rows
are exact. The kernels' own count of roundings is inside ``M + 16``
(``u_ij`` is exact here). Loss: 1 for ``w``, 2 for ``c (|u| - c / 2)``,
``M`` fused multiply-adds over ``j``, 2 for the factor ``1 / (kappa M)``
and its product, 6 butterfly steps and up to 3 additions over the waves:
``M + 14``. Gradient: 1 for ``w`` (the clamp is exact), ``M``
multiply-adds, 2 for the factor, 1 for the product with ``g_b``:
``M + 4``.

MEASURED on one MI355X, worst error / bound over all cases: loss 0.11,
gradient 0.98 (a bf16 case: the rounding of the store).
"""
import numpy as np
import pytest
import torch as t

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from util_quantile_loss import (  # noqa: E402
    MULTI_TRIP_SHAPE, all_cases, make_case, op_args, reference64, run_op,
    seeded_quantile_update, within_bound,
)

DEV = "cuda:0"


def run_device(case, kappa):
    return run_op(ops.quantile_huber_loss, case, kappa, DEV)


@all_cases
def test_within_the_bound(shape, tie, kappa, given_taus, dtype):
    case = make_case(shape, given_taus, dtype, tie)
    ref, bound = reference64(shape, given_taus, dtype, kappa, tie)
    result = run_device(case, kappa)
    assert all(x.is_cuda for x in result)
    assert within_bound(case, result, ref, bound, str(shape))
    if tie:  # two waves: the lower action, and two calls bit-equal
        assert t.equal(result[2].cpu(), case.want_best)
        for a, b in zip(result, run_device(case, kappa)):
            assert t.equal(a, b)


@pytest.mark.parametrize("kappa", [1.0, 0.0])
def test_more_samples_than_blocks(kappa):
    """The grid stops at 2048 blocks: the last three samples are done
    in a second trip of blocks 0 to 2."""
    case = make_case(MULTI_TRIP_SHAPE)
    ref, bound = reference64(MULTI_TRIP_SHAPE, False, t.float32, kappa)
    result = run_device(case, kappa)
    want = run_op(ops._quantile_huber_loss_torch, case, kappa)
    assert t.equal(result[1].cpu(), want[1])
    assert t.equal(result[2].cpu(), want[2])
    assert within_bound(case, result, ref, bound, "multi-trip")


def test_rejects_mixed_devices_and_the_binding_checks_itself():
    good = list(op_args(make_case((5, 3, 2, 200), True), 1.0, DEV))
    for i in (1, 2, 3, 4, 5, 6, 8):
        with pytest.raises(ValueError):
            ops.quantile_huber_loss(
                *good[:i], good[i].cpu(), *good[i + 1:])
    from machin_amd.ops import _machin_hip as ext

    # the binding takes (..., discount or None, scalar discount, kappa,
    # taus)
    good[6:8] = [None, 0.5, 1.0]
    for i, value in ((4, good[4].cpu()), (0, good[0].transpose(0, 1)),
                     (3, good[3][:, :, :100]), (8, -1.0),
                     (9, good[9][:, :1])):
        with pytest.raises(RuntimeError):
            ext.quantile_loss_fwd(*good[:i], value, *good[i + 1:])


def test_rainbow_update_matches_the_cpu():
    on_cpu, _, loss_cpu = seeded_quantile_update()
    on_gpu, before, loss_gpu = seeded_quantile_update(DEV)
    assert np.isfinite(loss_gpu)
    assert loss_gpu == pytest.approx(loss_cpu, rel=1e-4)
    for p, q, p0 in zip(on_cpu.qnet.parameters(),
                        on_gpu.qnet.parameters(), before):
        assert q.is_cuda and not t.equal(q, p0)
        assert t.allclose(p, q.cpu(), rtol=1e-4, atol=1e-6)
