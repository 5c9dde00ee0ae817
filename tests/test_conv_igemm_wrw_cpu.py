"""``ConvBiasReLU2d(impl="hip_wrw")`` where the implicit-GEMM kernels do
not apply: the call takes the library path, bit for bit."""
import pytest
import torch as t

from machin_amd.ops.fused_conv import ConvBiasReLU2d

DEVICES = ["cpu"] + (["cuda:0"] if t.cuda.is_available() else [])
# the ineligible calls of test_conv_igemm_cpu: (kernel, dtype, channels-last)
INELIGIBLE = {"fp32": (4, t.float32, True), "nchw": (4, t.bfloat16, False),
              "geometry": (5, t.bfloat16, True)}


def _run(mod, x):
    xi = x.clone().requires_grad_()
    y = mod(xi)
    y.backward(t.ones_like(y))
    return [y, xi.grad, mod.weight.grad, mod.bias.grad]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("why", INELIGIBLE)
def test_ineligible_calls_take_the_library_path(device, why, monkeypatch):
    k, dtype, channels_last = INELIGIBLE[why]
    t.manual_seed(0)
    wrw = ConvBiasReLU2d(32, 64, k, stride=2, impl="hip_wrw")
    ref = ConvBiasReLU2d(32, 64, k, stride=2, impl="miopen")
    env = ConvBiasReLU2d(32, 64, k, stride=2)
    ref.load_state_dict(wrw.state_dict())
    env.load_state_dict(wrw.state_dict())
    monkeypatch.setenv("MACHIN_CONV_IMPL", "hip_wrw")  # accepted
    x = t.randn(2, 32, 8, 8).to(device, dtype)
    if channels_last:
        x = x.contiguous(memory_format=t.channels_last)
    want = _run(ref.to(device, dtype), x)
    for mod in (wrw, env):
        for got, ref_v in zip(_run(mod.to(device, dtype), x), want):
            assert t.equal(got, ref_v)
