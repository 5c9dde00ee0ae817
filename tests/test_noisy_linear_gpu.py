"""The gfx950 NoisyLinear kernels (machin_amd/ops/hip/noisy_linear.hip)
against float64 references, the noise kernel's statistics, and the
modules and RAINBOW's ``noisy_nets`` option on the device.

The kernels are called through ``ops._NoisyLinear`` so that every shape
runs them whatever the dispatch limit of ``ops.noisy_linear`` is.

1. Exact: on small-integer inputs every product and partial sum is an
   integer below 2^24, so all six outputs must equal the float64
   reference bit for bit (a dropped or doubled term cannot hide).
2. Rounding: on normal inputs ``|got - ref| <= (K + 8) 2^-24 S`` per
   element (``util_noisy_linear.reference64``), plus ``2^-8 |ref|`` for
   a bf16 output.
"""
import copy
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch as t
import torch.nn as nn

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from machin_amd.frame.algorithms import RAINBOW  # noqa: E402
from machin_amd.frame.buffers import DeviceFrameStackBuffer  # noqa: E402
from machin_amd.model.nets import (  # noqa: E402
    NoisyDuelingC51Head, NoisyLinear, reset_noise,
)
from util_c51_loss import V_MAX, V_MIN, pixel_episode, seed_all  # noqa: E402
from util_noisy_linear import (  # noqa: E402
    BIG_SHAPES, OUTPUTS, SHAPE_IDS, SHAPES, SLICES, head_bound, make_case,
    reference64, run, shape_id, worst_ratio,
)

DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [t.float32, t.bfloat16],
                                 ids=["fp32", "bf16"])
ALL = pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
BIG = pytest.mark.parametrize("shape", BIG_SHAPES,
                              ids=[shape_id(s) for s in BIG_SHAPES])


def kernel(*args):
    return ops._NoisyLinear.apply(*args)


class TestKernels:
    def test_multi_step_shapes_loop(self):
        """The shapes meant to make a block run several reduction steps
        do so under the launchers' own slice policy."""
        ext = ops._require_ext()
        for (B, I, O), (fwd, dx) in SLICES.items():
            assert tuple(ext.noisy_linear_slices(B, O, I)) == fwd
            assert tuple(ext.noisy_linear_slices(B, I, O)) == dx
        # with and without slices, and a short last slice
        fwd, dx = zip(*SLICES.values())
        assert any(s > 1 and c > 1 for s, c in fwd + dx)
        assert any(s == 1 and c > 1 for s, c in fwd + dx)
        assert tuple(ext.noisy_linear_slices(1000, 100, 777)) == (7, 2)
        assert -(-777 // 64) % 2 == 1  # 13 steps in slices of 2

    @DTYPES
    @ALL
    def test_exact_on_integers(self, shape, dtype):
        case = make_case(shape, "int")
        ref, _ = reference64(shape, "int", dtype)
        got = run(kernel, case, dtype, DEV)
        assert got.y.dtype == got.dx.dtype == dtype
        for name in OUTPUTS:
            g, want = getattr(got, name).cpu(), getattr(ref, name)
            if name in ("y", "dx"):
                want = want.to(dtype)
            else:
                assert g.dtype == t.float32
            assert g.shape == want.shape, name
            assert t.equal(g.double(), want.double()), name

    @DTYPES
    @ALL
    def test_rounding_bound(self, shape, dtype):
        case = make_case(shape, "randn")
        ref, bound = reference64(shape, "randn", dtype)
        got = run(kernel, case, dtype, DEV)
        ratio, where = worst_ratio(got, ref, bound)
        print(f"{shape} {dtype}: worst |err| / bound = {ratio:.3f} ({where})")
        assert ratio <= 1.0, where

    @DTYPES
    @ALL
    def test_against_device_torch_form(self, shape, dtype):
        """Kernel and two-GEMM torch form on the device differ by at most
        twice the rounding bound (each is within one of the reference)."""
        case = make_case(shape, "randn")
        _, bound = reference64(shape, "randn", dtype)
        got = run(kernel, case, dtype, DEV)
        want = run(ops._noisy_linear_torch, case, dtype, DEV)
        for name in OUTPUTS:
            err = (getattr(got, name).double()
                   - getattr(want, name).double()).abs().cpu()
            assert bool((err <= 2 * getattr(bound, name)).all()), name

    @DTYPES
    @BIG
    def test_deterministic(self, shape, dtype):
        case = make_case(shape, "randn")
        one = run(kernel, case, dtype, DEV)
        two = run(kernel, case, dtype, DEV)
        for name in OUTPUTS:
            assert t.equal(getattr(one, name), getattr(two, name)), name

    @pytest.mark.parametrize("shape", [(33, 65, 17), (32, 3136, 512)],
                             ids=["33x65x17", "32x3136x512"])
    def test_no_input_gradient(self, shape):
        case = make_case(shape, "randn")
        full = run(kernel, case, t.float32, DEV)
        part = run(kernel, case, t.float32, DEV, x_grad=False)
        assert part.dx is None
        for name in OUTPUTS:
            if name != "dx":
                assert t.equal(getattr(part, name), getattr(full, name)), name

    def test_dispatch(self, monkeypatch):
        """Up to the batch limit ``ops.noisy_linear`` runs the kernels,
        above it the device torch form, bit for bit."""
        limit = ops.NOISY_LINEAR_FUSED_MAX_BATCH
        used = []
        real = ops._NoisyLinear.apply
        monkeypatch.setattr(ops._NoisyLinear, "apply",
                            lambda *a: used.append(1) or real(*a))
        for batch, fused in ((limit, True), (limit + 1, False)):
            case = make_case((batch, 65, 17), "randn")
            used.clear()
            got = run(ops.noisy_linear, case, t.float32, DEV)
            assert bool(used) == fused
            want = run(kernel if fused else ops._noisy_linear_torch, case,
                       t.float32, DEV)
            for name in OUTPUTS:
                assert t.equal(getattr(got, name), getattr(want, name)), name

    def test_autocast_region(self):
        """A forward inside a bf16 autocast region (the backward outside
        it, as autocast is meant to be used) still computes in fp32 on
        both device paths: same bits as without autocast, below and
        above the limit."""
        limit = ops.NOISY_LINEAR_FUSED_MAX_BATCH

        def in_region(*args):
            with t.autocast(device_type="cuda", dtype=t.bfloat16):
                return ops.noisy_linear(*args)

        for batch in (limit, limit + 1):
            case = make_case((batch, 65, 17), "randn")
            want = run(ops.noisy_linear, case, t.float32, DEV)
            got = run(in_region, case, t.float32, DEV)
            for name in OUTPUTS:
                assert t.equal(getattr(got, name), getattr(want, name)), name

    def test_leading_dimensions_and_views(self):
        case = make_case((7, 64, 64), "randn")
        args = [getattr(case, n).to(DEV) for n in (
            "weight_mu", "weight_sigma", "bias_mu", "bias_sigma", "eps_in",
            "eps_out")]
        x = case.x.to(DEV)
        flat = kernel(x, *args)
        wide = t.zeros(7, 2, 64, device=DEV)
        wide[:, 0] = x
        assert t.equal(kernel(wide[:, 0], *args), flat)
        assert t.equal(kernel(x.view(7, 1, 64), *args), flat.view(7, 1, 64))

    def test_rejects_bad_arguments(self):
        case = make_case((2, 3, 5), "randn")
        names = ("x", "weight_mu", "weight_sigma", "bias_mu", "bias_sigma",
                 "eps_in", "eps_out")
        good = {n: getattr(case, n).to(DEV) for n in names}
        ops.noisy_linear(**good)
        for change in (
            dict(x=good["x"].half()), dict(x=good["x"][:, :2]),
            dict(weight_mu=case.weight_mu),  # on the CPU
            dict(eps_in=good["eps_out"]),
            dict(bias_sigma=good["bias_sigma"].double()),
        ):
            with pytest.raises(ValueError):
                ops.noisy_linear(**{**good, **change})


class TestNoiseKernel:
    def test_statistics(self):
        n = 2 ** 20
        a = ops.factorised_noise_(t.empty(n, device=DEV), 3, 5)
        assert bool(t.isfinite(a).all())
        mean, second = float(a.double().mean()), float((a.double() ** 2).mean())
        print(f"mean {mean:.2e}, mean(e^2) - sqrt(2/pi) "
              f"{second - math.sqrt(2 / math.pi):.2e}")
        assert abs(mean) <= 5.3e-3
        assert abs(second - math.sqrt(2 / math.pi)) <= 3.6e-3
        # f(z) of a normal z: about half negative, |e| = sqrt|z|
        assert abs(float((a < 0).float().mean()) - 0.5) <= 3e-3

    def test_streams(self):
        n = 2 ** 20
        a = ops.factorised_noise_(t.empty(n, device=DEV), 3, 5)
        assert t.equal(a, ops.factorised_noise_(t.empty(n, device=DEV), 3, 5))
        for seed, offset in ((3, 6), (4, 5), (3, 5 + (1 << 16))):
            b = ops.factorised_noise_(t.empty(n, device=DEV), seed, offset)
            assert float((a == b).float().mean()) < 0.01
        # a prefix of a longer draw: elements are keyed by their index
        short = ops.factorised_noise_(t.empty(4097, device=DEV), 3, 5)
        assert t.equal(short, a[:4097])

    @pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
    def test_guard_element_stays(self, n):
        buf = t.full((n + 1,), 77.0, device=DEV)
        out = ops.factorised_noise_(buf[:n], 9, 1)
        assert out.data_ptr() == buf.data_ptr()
        assert float(buf[n]) == 77.0
        assert bool((buf[:n] != 77.0).all())
        assert bool(t.isfinite(buf).all())


class TestModulesOnDevice:
    def test_layer_against_reference(self):
        """A layer holding a case's parameters and noise, on the CPU and
        moved to the device (batch 31: the kernels), gives the case's
        float64 outputs within the rounding bound."""
        shape = (31, 63, 33)
        case = make_case(shape, "randn")
        ref, bound = reference64(shape, "randn", t.float32)
        layer = NoisyLinear(63, 33)
        with t.no_grad():
            for name in ("weight_mu", "weight_sigma", "bias_mu",
                         "bias_sigma"):
                getattr(layer, name).copy_(getattr(case, name))
            layer.eps.copy_(t.cat([case.eps_in, case.eps_out]))
        on_device = copy.deepcopy(layer).to(DEV)
        assert on_device.eps.is_cuda and t.equal(on_device.eps.cpu(),
                                                 layer.eps)
        assert on_device.eps_in.data_ptr() == on_device.eps.data_ptr()
        for module, device in ((layer, "cpu"), (on_device, DEV)):
            x = case.x.clone().to(device).requires_grad_(True)
            y = module(x)
            y.backward(case.dy.to(device))
            got = SimpleNamespace(
                y=y, dx=x.grad, dmu=module.weight_mu.grad,
                dsigma=module.weight_sigma.grad,
                dbias_mu=module.bias_mu.grad,
                dbias_sigma=module.bias_sigma.grad,
            )
            ratio, where = worst_ratio(got, ref, bound)
            assert ratio <= 1.0, (device, where)
        reset_noise(on_device, seed=5)
        assert not t.equal(on_device.eps.cpu(), layer.eps)
        assert not any("eps" in k for k in on_device.state_dict())

    @DTYPES
    def test_head_against_float64(self, dtype):
        """The head on the device, fed an fp32 or a bf16 feature, against
        the same head in float64 on the CPU with the noise copied over
        (see ``head_bound``). With a bf16 feature the bf16 kernels run
        and the logits still come out fp32."""
        seed_all(0)
        head = NoisyDuelingC51Head(64, 3, 11, hidden=40)
        on_device = copy.deepcopy(head).to(DEV)
        exact = copy.deepcopy(head).double()
        feat = t.randn(9, 64).to(dtype)
        x = feat.to(DEV).requires_grad_(True)
        got = on_device(x)
        assert got.dtype == t.float32 and got.shape == (9, 3, 11)
        got.sum().backward()
        assert x.grad.dtype == dtype
        assert bool(t.isfinite(x.grad.float()).all())
        want = exact(feat.double()).detach()
        bound = head_bound(exact, feat.double(), dtype)
        assert bool(((got.detach().cpu().double() - want).abs()
                     <= bound).all())


class PixelNoisyQNet(nn.Module):
    """Tiny noisy dueling C51 net on [B, 4, 16, 16] u8 stacks: logits."""

    def __init__(self, action_num=3, atom_num=11):
        super().__init__()
        self.torso = nn.Linear(4 * 16 * 16, 32)
        self.head = NoisyDuelingC51Head(32, action_num, atom_num, hidden=24)

    def forward(self, state):
        feat = t.relu(self.torso(state.float().flatten(1) / 255.0))
        return self.head(feat)


class TestRainbowOnDevice:
    def test_update_on_framestack_replay(self):
        seed_all(0)
        buf = DeviceFrameStackBuffer(
            200, DEV, n_step=3, discount=0.9, prioritized=True
        )
        algo = RAINBOW(
            PixelNoisyQNet().to(DEV), PixelNoisyQNet().to(DEV),
            t.optim.Adam, V_MIN, V_MAX, batch_size=8,
            reward_future_steps=3, discount=0.9, replay_buffer=buf,
            fused_loss=True, dist_from_logits=True, noisy_nets=True,
        )
        for seed, length in enumerate((7, 5, 9)):
            algo.store_episode(pixel_episode(length, 16, 16, seed=seed))
        noise = algo.qnet.head.value_out.eps.clone()
        sigma = algo.qnet.head.value_out.weight_sigma.detach().clone()
        loss = algo.update()
        assert np.isfinite(loss)
        for net in (algo.qnet, algo.qnet_target):
            for p in net.parameters():
                assert bool(t.isfinite(p).all())
        assert not t.equal(algo.qnet.head.value_out.eps, noise)
        assert not t.equal(algo.qnet.head.value_out.weight_sigma, sigma)
        state = {"state": t.randint(0, 256, (5, 4, 16, 16), dtype=t.uint8,
                                    device=DEV)}
        epsilon = algo.epsilon
        action = algo.act_discrete_with_noise(state)
        assert action.shape == (5, 1) and action.dtype == t.int64
        assert action.is_cuda and algo.epsilon == epsilon
        assert algo.act_discrete(state).shape == (5, 1)
