"""CPU fallback of the conv + bias + ReLU module."""
import torch as t
import torch.nn.functional as F


def test_conv_bias_relu_fallback_matches_torch():
    from machin_amd.ops.fused_conv import ConvBiasReLU2d, bias_relu

    t.manual_seed(0)
    conv = ConvBiasReLU2d(8, 16, 3, stride=2)
    assert [n for n, _ in conv.named_parameters()] == ["weight", "bias"]
    x = t.randn(2, 8, 9, 9, requires_grad=True)
    y = conv(x)
    ref = F.relu(F.conv2d(x, conv.weight, conv.bias, stride=2))
    # fp32: the bias joins after the accumulation instead of inside it,
    # at most a couple of roundings of an O(1) value
    assert t.allclose(y, ref, rtol=0.0, atol=1e-6)
    assert ((y == 0) == (ref == 0)).all()
    go = t.randn_like(ref)
    got = t.autograd.grad(y, [x, conv.weight, conv.bias], go)
    exp = t.autograd.grad(ref, [x, conv.weight, conv.bias], go)
    for a, b in zip(got, exp):
        assert t.allclose(a, b, rtol=1e-5, atol=1e-5)

    # the bare op on a plain tensor
    z = t.randn(2, 16, 4, 4)
    assert t.equal(bias_relu(z, conv.bias),
                   F.relu(z + conv.bias.view(1, -1, 1, 1)))


def test_flatten_option_of_the_fallback():
    from machin_amd.ops.fused_conv import ConvBiasReLU2d

    t.manual_seed(1)
    conv = ConvBiasReLU2d(8, 16, 3, flatten=True)
    x = t.randn(2, 8, 5, 5)
    ref = F.relu(F.conv2d(x, conv.weight, conv.bias)).flatten(1)
    assert conv(x).shape == (2, 16 * 3 * 3)
    assert t.allclose(conv(x), ref, rtol=0.0, atol=1e-6)
