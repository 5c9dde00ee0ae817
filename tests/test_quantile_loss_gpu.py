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

General inputs (``make_general_case``, ``general_reference``): normal
values at three scales, a per-sample discount, any ``kappa``. ``target``
is bit-equal to the correctly rounded fp32 definition; loss and gradient
lie within ``(M + 20) 2^-24`` times the magnitude sums of a float64
reference formed from it (count in ``util_quantile_loss``), the kernel
and the torch fallback within twice that of each other. The same checks
run on the fallback in ``test_quantile_loss_cpu``.

MEASURED on one MI355X, worst error / bound over the 360 general cases:
loss 0.10 (fp32) and 0.08 (bf16), gradient 0.24 (fp32) and 0.99 (bf16:
the rounding of the store). Before the target's product and sum were
kept from contracting to one fma, ``target`` missed the fp32 definition
in all 360 cases and the gradient at a planted ``u = 0`` reached
7.6e5 bounds.
"""
import numpy as np
import pytest
import torch as t

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from util_quantile_loss import (  # noqa: E402
    CONTAINMENT_SHAPE, GENERAL_MULTI_TRIP_SHAPE, MULTI_TRIP_SHAPE,
    NON_FINITE, all_cases, check_bf16_gradient_overflow,
    check_nonfinite_online, check_permutation, check_poisoned_sample,
    check_reductions, check_scalar_discount, check_views, general_cases,
    general_reference64, make_case, make_general_case, op_args, reference64,
    run_op, same_bits, seeded_quantile_update, within_bound,
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


def on_fallback(case, kappa, result, bound):
    """Kernel against the torch fallback on finite inputs: ``target`` and
    ``best`` bit-equal, loss and gradient within twice the bound (each
    is within one bound of float64)."""
    B, A, N, M = case.shape
    want = run_op(ops.quantile_huber_loss, case, kappa)
    rows, a_b = t.arange(B), case.action.clamp(0, A - 1)
    assert same_bits(result[1], want[1]) and same_bits(result[2], want[2])
    for got, ref, limit in (
            (result[0], want[0], bound.loss),
            (result[3][rows, a_b], want[3][rows, a_b], bound.grad)):
        err = (got.cpu().double() - ref.double()).abs()
        assert bool((err <= 2.0 * limit).all())


@general_cases
def test_within_the_bound_on_general_inputs(
        shape, kappa, scale, given_taus, dtype):
    """``target`` bit-equal to the fp32 definition, loss and gradient
    within ``(M + 20) 2^-24 S`` of float64 (``general_reference``)."""
    case = make_general_case(shape, given_taus, dtype, scale)
    ref, bound = general_reference64(shape, given_taus, dtype, scale, kappa)
    result = run_device(case, kappa)
    assert all(x.is_cuda for x in result)
    assert within_bound(case, result, ref, bound,
                        f"general {shape} {kappa} {scale} {dtype}")
    on_fallback(case, kappa, result, bound)


@pytest.mark.parametrize("kappa", [1.0, 0.0])
def test_more_samples_than_blocks_with_several_waves(kappa):
    """bf16, given fractions, two waves and more actions than waves: the
    second trip reuses ``q_s``, ``t_s`` and ``part_s`` for samples with
    other discounts, actions and terminals."""
    shape = GENERAL_MULTI_TRIP_SHAPE
    case = make_general_case(shape, True, t.bfloat16)
    ref, bound = general_reference64(shape, True, t.bfloat16, 1.0, kappa)
    result = run_device(case, kappa)
    assert within_bound(case, result, ref, bound, "general multi-trip")
    on_fallback(case, kappa, result, bound)


@pytest.mark.parametrize("dtype", [t.float32, t.bfloat16], ids=str)
@pytest.mark.parametrize("given_taus", [False, True])
@pytest.mark.parametrize("kappa", [1.0, 0.0])
def test_follows_a_permutation_of_the_samples(kappa, given_taus, dtype):
    case = make_general_case((7, 3, 65, 33), given_taus, dtype)
    check_permutation(ops.quantile_huber_loss, DEV, case, kappa)


@pytest.mark.parametrize("shape,dtype", [
    ((5, 2, 6, 7), t.float32), ((5, 2, 6, 7), t.bfloat16),
    (GENERAL_MULTI_TRIP_SHAPE, t.bfloat16)], ids=str)
@pytest.mark.parametrize("kappa", [0.1, 0.0])
def test_scalar_discount(shape, dtype, kappa):
    case = make_general_case(shape, True, dtype)
    check_scalar_discount(ops.quantile_huber_loss, DEV, case, kappa)


@pytest.mark.parametrize("dtype", [t.float32, t.bfloat16], ids=str)
def test_as_it_is_called(dtype):
    case = make_general_case((7, 3, 65, 33), True, dtype)
    check_reductions(ops.quantile_huber_loss, DEV, case, 1.0)
    check_views(ops.quantile_huber_loss, DEV, case, 1.0)


@pytest.mark.parametrize("dtype", [t.float32, t.bfloat16], ids=str)
@pytest.mark.parametrize("kappa", [1.0, 0.0])
def test_best_with_non_finite_row_sums(kappa, dtype):
    case = make_general_case((7, 3, 65, 33), False, dtype)
    result = check_nonfinite_online(ops.quantile_huber_loss, DEV, case, kappa)
    dirty = check_nonfinite_online(
        ops.quantile_huber_loss, "cpu", case, kappa)
    assert same_bits(result[1], dirty[1]) and same_bits(result[2], dirty[2])


@pytest.mark.parametrize("dtype", [t.float32, t.bfloat16], ids=str)
@pytest.mark.parametrize("kappa", [1.0, 0.0])
@pytest.mark.parametrize("what,b", NON_FINITE)
def test_non_finite_sample(what, b, kappa, dtype):
    """For ``theta = +-inf`` the gradient follows the definition here:
    finite and within the bound."""
    case = make_general_case((7, 3, 65, 33), True, dtype)
    result = check_poisoned_sample(
        ops.quantile_huber_loss, DEV, case, kappa, what, b)
    if dtype == t.bfloat16 and not what.startswith("theta_"):
        a_b = int(case.action[b].clamp(0, case.shape[1] - 1))
        raw = result[3][b, a_b].cpu().view(t.int16).int() & 0x7fff
        assert bool((raw[-1:] > 0x7f80).all())  # a bf16 NaN, not inf


@pytest.mark.parametrize("b", [1, 2049])
def test_contains_a_nan_in_a_second_trip(b):
    """Block 1 does samples 1 and 2049: a NaN in ``q_s``, ``t_s`` and
    ``part_s`` of either trip stays in its sample."""
    case = make_general_case(CONTAINMENT_SHAPE, False, t.bfloat16)
    check_poisoned_sample(ops.quantile_huber_loss, DEV, case, 1.0,
                          "online_and_reward", b)


def test_bf16_gradient_overflows_to_infinity():
    check_bf16_gradient_overflow(ops.quantile_huber_loss, DEV)


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
