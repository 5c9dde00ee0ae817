"""Fused bias / ReLU kernels of the Atari conv stack against the torch
composition they replace: the stem's ReLU epilogue and packed sign
mask, the masked weight-gradient kernel, the conv2/conv3 bias+ReLU
pair, and the whole fused model."""
import math

import pytest
import torch as t
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
SCALE = 1.0 / 255.0
# the stem weight gradient is a split-K sum of fp32 atomics: two
# evaluations of the same sum differ only by reordering
ATOMIC_RTOL = 1e-5


def _ext():
    from machin_amd.ops import _require_ext

    return _require_ext()


def _frames_nhwc(batch, seed):
    g = t.Generator(device=DEV).manual_seed(seed)
    return t.randint(0, 256, (batch, 84, 84, 4), dtype=t.uint8,
                     device=DEV, generator=g)


def _stem_weights(seed):
    g = t.Generator(device=DEV).manual_seed(seed)
    w = t.randn(32, 4, 8, 8, device=DEV, generator=g) * 0.05
    b = t.randn(32, device=DEV, generator=g) * 0.1
    w_rs = w.permute(2, 3, 1, 0).reshape(256, 32).to(
        t.bfloat16
    ).contiguous()
    return w, b, w_rs


def _unpack_mask(mask):
    """[K] int32 words -> [K, 32] bool, bit c of word k at [k, c]."""
    shifts = t.arange(32, device=mask.device, dtype=t.int32)
    return ((mask.view(-1, 1) >> shifts) & 1).bool()


def _assert_atomic_close(got, ref, what):
    bound = ATOMIC_RTOL * ref.abs().max().item()
    diff = (got.float() - ref.float()).abs().max().item()
    print(f"{what}: max abs diff {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound, f"{what}: {diff} > {bound}"


def _bf16_ulp(x):
    """Spacing of bf16 (8 significand bits) at |x|, elementwise."""
    ax = x.abs().double().clamp_min(2.0 ** -126)
    return t.pow(2.0, t.floor(t.log2(ax)) - 7)


def _assert_within_one_bf16_ulp(got, ref, what):
    got, ref = got.double(), ref.double()
    ulp = _bf16_ulp(t.maximum(got.abs(), ref.abs()))
    worst = ((got - ref).abs() / ulp).max().item()
    print(f"{what}: worst difference {worst:.3f} bf16 ulp")
    assert worst <= 1.0, f"{what}: {worst} ulp"


class TestStemForward:
    # batch 3: K = 1200 = 9*128 + 48 -> partial last workgroup
    @pytest.mark.parametrize("batch", [1, 3])
    def test_relu_and_mask(self, batch):
        ext = _ext()
        frames = _frames_nhwc(batch, 10 + batch)
        _, b, w_rs = _stem_weights(3)
        plain = ext.conv1_fwd(frames, w_rs, b, SCALE)
        y, mask = ext.conv1_fwd_relu(frames, w_rs, b, SCALE)
        assert y.shape == (batch * 400, 32) and y.dtype == t.bfloat16
        assert mask.shape == (batch * 400,) and mask.dtype == t.int32
        assert t.equal(y, t.relu(plain))
        assert t.equal(_unpack_mask(mask), y > 0)
        # both signs must occur for the check to mean anything
        frac = (y > 0).float().mean().item()
        assert 0.2 < frac < 0.8, frac


class TestStemWeightGrad:
    # batch 1: K = 400 = 6*64 + 16 (chunk tail), split-K over 7 groups
    @pytest.mark.parametrize("batch", [1, 3])
    @pytest.mark.parametrize("kind", ["random", "clear", "set"])
    def test_masked_matches_premasked(self, batch, kind):
        ext = _ext()
        K = batch * 400
        frames = _frames_nhwc(batch, 20 + batch)
        g = t.Generator(device=DEV).manual_seed(7)
        dy = (t.randn(K, 32, device=DEV, generator=g) * 0.1).to(
            t.bfloat16
        )
        if kind == "random":
            mask = t.randint(-2 ** 31, 2 ** 31, (K,), device=DEV,
                             generator=g, dtype=t.int64).to(t.int32)
        elif kind == "clear":
            mask = t.zeros(K, dtype=t.int32, device=DEV)
        else:
            mask = t.full((K,), -1, dtype=t.int32, device=DEV)
        gw, gb = ext.conv1_wrw_masked(dy, mask, frames, SCALE)
        dy_ref = (dy * _unpack_mask(mask).to(t.bfloat16)).contiguous()
        ref_w, ref_b = ext.conv1_wrw(dy_ref, frames, SCALE)
        if kind == "clear":
            assert t.equal(gw, t.zeros_like(gw))
            assert t.equal(gb, t.zeros_like(gb))
            return
        _assert_atomic_close(gw, ref_w, f"grad_w {kind} B={batch}")
        _assert_atomic_close(gb, ref_b, f"grad_b {kind} B={batch}")


class TestStemModule:
    def test_relu_flag_matches_composition(self):
        from machin_amd.ops.fused_conv import FusedAtariConv1

        B = 4
        frames = _frames_nhwc(B, 31).permute(0, 3, 1, 2)
        fused = FusedAtariConv1(relu=True).to(DEV)
        plain = FusedAtariConv1(relu=False).to(DEV)
        plain.load_state_dict(fused.state_dict())
        g = t.Generator(device=DEV).manual_seed(5)
        go = t.randn(B, 32, 20, 20, device=DEV, generator=g).to(
            t.bfloat16
        ).contiguous(memory_format=t.channels_last)

        y = fused(frames)
        y_ref = t.relu(plain(frames))
        assert t.equal(y, y_ref)
        y.backward(go)
        y_ref.backward(go)
        _assert_atomic_close(fused.weight.grad, plain.weight.grad,
                             "stem weight grad")
        _assert_atomic_close(fused.bias.grad, plain.bias.grad,
                             "stem bias grad")

    def test_retired_kernels_take_the_unfused_path(self, monkeypatch):
        from machin_amd.ops.fused_conv import FusedAtariConv1

        frames = _frames_nhwc(2, 32).permute(0, 3, 1, 2)
        stem = FusedAtariConv1(relu=True).to(DEV)
        y3 = stem(frames)
        monkeypatch.setenv("MACHIN_CONV1_V", "1")
        y1 = stem(frames)
        assert (y1 >= 0).all()
        # v1 and v3 order the K reduction differently: bf16 rounding
        assert t.allclose(y1.float(), y3.float(), rtol=2e-2, atol=2e-2)


# (R, C): rows below / at / above one block's 32-row pass, several
# blocks with a partial last one, more rows than one pass of the capped
# grid (grid-stride and multi-pass paths), and channel counts that
# leave idle lanes (C=24) or need several finishing sweeps (C=320)
BIAS_ACT_SHAPES = [
    (7, 64), (81, 64), (3 * 49, 64), (4099, 64), (131109, 64),
    (4099, 24), (4099, 320),
]


def _bias_act_inputs(R, C):
    g = t.Generator(device=DEV).manual_seed(R * 31 + C)
    y = t.randn(R, C, device=DEV, generator=g).to(t.bfloat16)
    bias = t.randn(C, device=DEV, generator=g) * 0.5
    gy = t.randn(R, C, device=DEV, generator=g).to(t.bfloat16)
    return y, bias, gy


class TestBiasRelu:
    @pytest.mark.parametrize("R,C", BIAS_ACT_SHAPES)
    def test_forward_bit_exact(self, R, C):
        ext = _ext()
        y, bias, _ = _bias_act_inputs(R, C)
        ref = t.relu(
            (y.float() + bias.to(t.bfloat16).float()).to(t.bfloat16)
        )
        # what autocast + ATen compute for the same expression
        ref_aten = t.relu(y.clone().add_(bias.to(t.bfloat16).view(1, -1)))
        assert t.equal(ref, ref_aten)
        out = y.clone()
        ext.bias_relu_(out, bias)
        assert t.equal(out, ref)

    @pytest.mark.parametrize("R,C", BIAS_ACT_SHAPES)
    def test_backward(self, R, C):
        ext = _ext()
        y, bias, gy = _bias_act_inputs(R, C)
        act = y.clone()
        ext.bias_relu_(act, bias)
        gx, gb = ext.bias_relu_bwd(gy, act)
        assert gb.dtype == t.float32 and gb.shape == (C,)
        ref_gx = t.ops.aten.threshold_backward(gy, act, 0)
        assert t.equal(gx, ref_gx)
        ref_gb = ref_gx.double().sum(0).to(t.bfloat16)
        assert t.equal(gb, gb.to(t.bfloat16).float()), "not bf16-rounded"
        _assert_within_one_bf16_ulp(gb, ref_gb, f"bias grad R={R} C={C}")
        gx2, gb2 = ext.bias_relu_bwd(gy, act)
        assert t.equal(gx, gx2) and t.equal(gb, gb2)

    def test_module_matches_conv_bias_relu(self):
        from machin_amd.ops.fused_conv import ConvBiasReLU2d

        conv = ConvBiasReLU2d(32, 64, 4, stride=2).to(DEV).to(
            memory_format=t.channels_last
        )
        g = t.Generator(device=DEV).manual_seed(2)
        x = t.randn(3, 32, 20, 20, device=DEV, generator=g).to(
            t.bfloat16
        ).contiguous(memory_format=t.channels_last).requires_grad_(True)
        with t.autocast(device_type="cuda", dtype=t.bfloat16):
            y = conv(x)
            ref = F.relu(F.conv2d(x, conv.weight, conv.bias, stride=2))
        assert t.equal(y, ref)
        go = t.randn(y.shape, device=DEV, generator=g).to(t.bfloat16)
        gx, gw, gb = t.autograd.grad(y, [x, conv.weight, conv.bias], go)
        rx, rw, rb = t.autograd.grad(ref, [x, conv.weight, conv.bias], go)
        assert gb.dtype == t.float32
        _assert_within_one_bf16_ulp(gb, rb, "module bias grad")
        assert t.equal(gx, rx)
        # MIOpen's weight gradient may sum split-K partials with fp32
        # atomics before rounding to bf16: one bf16 step (2^-8) of the
        # largest element bounds a rounding flip
        bound = 2.0 ** -8 * rw.abs().max().item()
        assert (gw - rw).abs().max().item() <= bound


class TestBiasReluFlat:
    # (N, C, H, W): the model's conv3 shape (one 16 B piece pass plus a
    # partial one), more samples than blocks of the capped grid, a
    # single pixel, and channel counts with idle lanes / several sweeps
    SHAPES = [(3, 64, 7, 7), (2051, 64, 7, 7), (5, 64, 1, 1),
              (4, 24, 5, 3), (2, 320, 3, 3)]

    @pytest.mark.parametrize("N,C,H,W", SHAPES)
    def test_forward_and_backward(self, N, C, H, W):
        ext = _ext()
        g = t.Generator(device=DEV).manual_seed(N * 7 + C)
        y = t.randn(N, C, H, W, device=DEV, generator=g).to(
            t.bfloat16
        ).contiguous(memory_format=t.channels_last)
        bias = t.randn(C, device=DEV, generator=g) * 0.5
        rows = y.permute(0, 2, 3, 1).reshape(-1, C)
        ref = t.relu(y + bias.to(t.bfloat16).view(1, -1, 1, 1))
        out = ext.bias_relu_flat(rows, bias, N)
        assert out.shape == (N, C * H * W)
        assert t.equal(out, ref.flatten(1))

        gy = t.randn(N, C * H * W, device=DEV, generator=g).to(t.bfloat16)
        gx, gb = ext.bias_relu_flat_bwd(gy, out, C)
        ref_gx = t.ops.aten.threshold_backward(
            gy.view(N, C, H, W), ref, 0
        )
        assert t.equal(gx.view(N, H, W, C).permute(0, 3, 1, 2), ref_gx)
        ref_gb = ref_gx.double().sum((0, 2, 3)).to(t.bfloat16)
        assert t.equal(gb, gb.to(t.bfloat16).float()), "not bf16-rounded"
        _assert_within_one_bf16_ulp(gb, ref_gb, f"flat bias grad N={N}")
        gx2, gb2 = ext.bias_relu_flat_bwd(gy, out, C)
        assert t.equal(gx, gx2) and t.equal(gb, gb2)


def _reference_forward(params, frames):
    """Today's unfused composition, from torch ops and the plain stem
    kernel, with the same parameters."""
    from machin_amd.ops.fused_conv import _FusedConv1Fn

    x = t.relu(_FusedConv1Fn.apply(
        frames, params["stem.weight"], params["stem.bias"], SCALE, False
    ))
    with t.autocast(device_type="cuda", dtype=t.bfloat16):
        x = F.relu(F.conv2d(x, params["conv_rest.0.weight"],
                            params["conv_rest.0.bias"], stride=2))
        x = F.relu(F.conv2d(x, params["conv_rest.2.weight"],
                            params["conv_rest.2.bias"], stride=1))
        feat = F.relu(F.linear(x.flatten(1), params["fc.1.weight"],
                               params["fc.1.bias"]))
        return (
            F.linear(feat, params["policy.weight"], params["policy.bias"]),
            F.linear(feat, params["value.weight"], params["value.bias"]),
        )


class TestWholeModel:
    def test_matches_unfused_composition(self):
        from machin_amd.model.nets.nature_cnn import FusedActorCriticCNN

        B = 6
        net = FusedActorCriticCNN(action_num=3).to(DEV).to(
            memory_format=t.channels_last
        )
        assert [n for n, _ in net.named_parameters()] == [
            "stem.weight", "stem.bias",
            "conv_rest.0.weight", "conv_rest.0.bias",
            "conv_rest.2.weight", "conv_rest.2.bias",
            "fc.1.weight", "fc.1.bias",
            "policy.weight", "policy.bias",
            "value.weight", "value.bias",
        ]
        params = {
            n: p.detach().clone().requires_grad_(True)
            for n, p in net.named_parameters()
        }
        frames = _frames_nhwc(B, 41).permute(0, 3, 1, 2)
        g = t.Generator(device=DEV).manual_seed(9)
        g_logits = t.randn(B, 3, device=DEV, generator=g)
        g_values = t.randn(B, 1, device=DEV, generator=g)

        def loss_of(logits, values):
            return ((logits.float() * g_logits).sum()
                    + (values.float() * g_values).sum())

        logits, values = net(frames)
        ref_logits, ref_values = _reference_forward(params, frames)
        assert t.equal(logits, ref_logits)
        assert t.equal(values, ref_values)
        loss_of(logits, values).backward()
        loss_of(ref_logits, ref_values).backward()
        for name, p in net.named_parameters():
            ref = params[name].grad
            assert p.grad is not None and ref is not None, name
            assert ref.abs().max().item() > 0, name
            if name in ("conv_rest.0.bias", "conv_rest.2.bias"):
                # deterministic fp32 sum in another order than ATen's,
                # then rounded to bf16: a rounding-boundary flip
                _assert_within_one_bf16_ulp(p.grad, ref, name)
            else:
                _assert_atomic_close(p.grad, ref, name)
        assert math.isfinite(loss_of(logits, values).item())
