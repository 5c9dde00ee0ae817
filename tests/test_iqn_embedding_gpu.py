"""GPU tests of the fused IQN cosine tau-embedding kernels against the
float64 reference and the derived bound of ``util_iqn``, and ``IQN`` on
``cuda:0``.

MEASURED on one MI355X, worst error / bound per case: (1,1,1,1) fp32 0.000
(``cos(0)`` is exact); (3,5,70,64) fp32 0.081 (dbias), bf16 0.940 (h: the
rounding of the store); (2,33,130,64) fp32 0.023 (dweight), bf16 0.949
(h); (5,8,64,6) fp32 0.135 (h); (2060,33,33,64) fp32 0.034 (h).
"""
import numpy as np
import pytest
import torch as t

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from machin_amd.ops import _iqn_embedding_torch  # noqa: E402
from util_iqn import (  # noqa: E402
    OUTPUTS, SHAPES, SLICED_SHAPE, make_case, reference64, run,
    seeded_iqn_update, worst_ratio,
)

DEV = "cuda:0"
F32, BF16 = t.float32, t.bfloat16
# the shapes of util_iqn; bf16 where a tile has more than its edge to show
CASES = [(SHAPES[0], F32), (SHAPES[1], F32), (SHAPES[1], BF16),
         (SHAPES[2], F32), (SHAPES[2], BF16), (SHAPES[3], F32),
         (SLICED_SHAPE, F32)]
cases = pytest.mark.parametrize("shape,dtype", CASES, ids=str)


def same_bits(a, b):
    return all(t.equal(getattr(a, n).view(t.uint8), getattr(b, n).view(t.uint8))
               for n in OUTPUTS)


@cases
def test_within_the_bound_and_of_the_composition(shape, dtype):
    ref, bound, ambiguous = reference64(shape, dtype)
    assert ambiguous <= 1e-3
    case = make_case(shape)
    got = run(ops.iqn_embedding, case, dtype, DEV)
    assert got.h.dtype == dtype and got.h.is_contiguous()
    ratio, where = worst_ratio(got, ref, bound)
    print(f"{shape} {dtype}: worst error / bound {ratio:.3f} ({where})")
    assert ratio <= 1.0, where
    # the torch form on the device: each within the bound of the
    # reference, so within twice the bound of each other
    torch_form = run(_iqn_embedding_torch, case, dtype, DEV)
    as_ref = type(ref)(**{n: getattr(torch_form, n).cpu().double()
                          for n in OUTPUTS})
    ratio, where = worst_ratio(got, as_ref, bound, scale=2.0)
    assert ratio <= 1.0, where
    # fixed order of every sum: a second call returns the same bits
    assert same_bits(got, run(ops.iqn_embedding, case, dtype, DEV))


@pytest.mark.parametrize("shape,dtype", CASES[1:], ids=str)
def test_permuting_the_samples_permutes_h_and_dpsi(shape, dtype):
    case = make_case(shape)
    perm = t.randperm(shape[0], generator=t.Generator().manual_seed(5))
    got = run(ops.iqn_embedding, case, dtype, DEV)
    moved = type(case)(**{**vars(case), "psi": case.psi[perm],
                          "taus": case.taus[perm], "dh": case.dh[perm]})
    other = run(ops.iqn_embedding, moved, dtype, DEV)
    perm = perm.to(DEV)
    assert t.equal(other.h.view(t.uint8), got.h[perm].view(t.uint8))
    assert t.equal(other.dpsi.view(t.uint8), got.dpsi[perm].view(t.uint8))


@pytest.mark.parametrize("shape,dtype", CASES[1:], ids=str)
def test_a_nan_stays_in_its_row_or_column(shape, dtype):
    case = make_case(shape)
    B, N, D, _ = shape
    b, n, d = B - 1, N // 2, D - 1
    taus, psi = case.taus.clone(), case.psi.clone()
    taus[b, n], psi[0, d] = float("nan"), float("nan")
    with t.no_grad():
        h = ops.iqn_embedding(psi.to(DEV, dtype), taus.to(DEV),
                              case.weight.to(DEV), case.bias.to(DEV)).cpu()
    want = t.zeros(B, N, D, dtype=t.bool)
    # 0 * NaN is a NaN as well: the whole row and the whole column
    want[b, n], want[0, :, d] = True, True
    clean = run(ops.iqn_embedding, case, dtype, DEV).h.cpu()
    assert t.equal(h.isnan(), want)
    assert t.equal(h[~want].view(t.uint8), clean[~want].view(t.uint8))


def test_rejects_mixed_devices_and_the_binding_checks_itself():
    case = make_case(SHAPES[1])
    good = [case.psi.to(DEV), case.taus.to(DEV), case.weight.to(DEV),
            case.bias.to(DEV)]
    for i in range(4):
        with pytest.raises(ValueError):
            ops.iqn_embedding(*good[:i], good[i].cpu(), *good[i + 1:])
    from machin_amd.ops import _machin_hip as ext

    wide = t.zeros(70, 65, device=DEV)
    for i, value in ((0, good[0].half()), (0, good[0].t().contiguous().t()),
                     (2, wide), (1, good[1].double()), (3, good[3].cpu())):
        with pytest.raises(RuntimeError):
            ext.iqn_embed_fwd(*good[:i], value, *good[i + 1:])
        with pytest.raises(RuntimeError):
            ext.iqn_embed_bwd(case.dh.to(DEV), *good[:i], value,
                              *good[i + 1:])


def test_iqn_update_matches_the_cpu():
    on_cpu, _, loss_cpu = seeded_iqn_update()
    on_gpu, before, loss_gpu = seeded_iqn_update(DEV)
    assert np.isfinite(loss_gpu)
    assert loss_gpu == pytest.approx(loss_cpu, rel=1e-4)
    for p, q, p0 in zip(on_cpu.qnet.parameters(),
                        on_gpu.qnet.parameters(), before):
        assert q.is_cuda and not t.equal(q, p0)
        assert t.allclose(p, q.cpu(), rtol=1e-4, atol=1e-6)
