"""The inputs and float64 references of ``util_stem_conv`` checked on the
CPU: the references against ``torch.autograd`` of a float64 conv, the
conditions that make the exact kinds exact, and the teeth of the GPU
tests that use them. The last part perturbs a float64 model of the
kernels the way a subtly wrong kernel would (a dropped tap, two swapped
taps, ties rounded away from zero, the mask bit set on ``y == 0``, one
border position read from the neighbouring row) and asserts that the
equality the GPU tests demand breaks."""
import math

import numpy as np
import pytest
import torch as t
import torch.nn.functional as F

from util_stem_conv import (
    BATCHES, EXACT_SCALES, F_MFMA, FORCED_BYTES, FWD_EXACT_KINDS, MASK_KINDS,
    MFMA_PROBE_MEASURED, ROUND_SCALE, dequant, forward_case, forward_reference, im2col,
    is_bf16_tie, pack_mask, probe_tiles, repack, round_bf16, rows,
    scale_tensor, tap_index, unpack_mask, worst_ratio, wrw_case,
    wrw_float64, wrw_mask, wrw_reference,
)

TAPS_KINDS = FWD_EXACT_KINDS[:8]
BOTH = pytest.mark.parametrize("with_bias", [True, False],
                               ids=["bias", "nobias"])
SCALES = pytest.mark.parametrize("scale", EXACT_SCALES, ids=["s1", "s2^-8"])
BATCH = pytest.mark.parametrize("batch", BATCHES)


def exact_cases():
    """(batch, kind): the taps sets at batch 3 only, as on the GPU."""
    out = [(3, k) for k in TAPS_KINDS]
    return out + [(b, k) for b in BATCHES for k in ("signs", "dense")]


EXACT = pytest.mark.parametrize("batch,kind", exact_cases())


class TestHelpers:
    def test_dequant_matches_numpy_float32(self):
        v = t.arange(256, dtype=t.uint8)
        got = dequant(v, ROUND_SCALE)
        assert got.dtype == t.bfloat16
        prod = v.numpy().astype(np.float32) * np.float32(1.0 / 255.0)
        assert prod.dtype == np.float32
        want = t.from_numpy(prod).to(t.bfloat16)
        assert t.equal(got, want)
        assert float(scale_tensor(1.0 / 255.0)) == ROUND_SCALE
        # and bf16 of a float32 is the one rounding round_bf16 does
        assert t.equal(got.double(), round_bf16(t.from_numpy(prod).double()))

    @SCALES
    def test_exact_scales_dequantise_exactly(self, scale):
        v = t.arange(256, dtype=t.uint8)
        assert t.equal(dequant(v, scale).double(), v.double() * scale)

    def test_repack_is_the_tap_formula(self):
        w = t.arange(32 * 4 * 8 * 8, dtype=t.float32).view(32, 4, 8, 8)
        w_rs = repack(w)
        assert w_rs.shape == (256, 32)
        for ky in range(8):
            for kx in range(8):
                for ci in range(4):
                    n = tap_index(ky, kx, ci)
                    assert n == (ky * 8 + kx) * 4 + ci
                    assert t.equal(w_rs[n], w[:, ci, ky, kx])

    def test_im2col_is_the_tap_formula(self):
        x = t.arange(2 * 84 * 84 * 4, dtype=t.float64).view(2, 84, 84, 4)
        cols = im2col(x)
        assert cols.shape == (800, 256)
        for b, oh, ow, ky, kx, ci in [(0, 0, 0, 0, 0, 0), (1, 19, 19, 7, 7, 3),
                                      (1, 3, 17, 2, 5, 1), (0, 19, 0, 7, 0, 2)]:
            assert cols[(b * 20 + oh) * 20 + ow, tap_index(ky, kx, ci)] \
                == x[b, oh * 4 + ky, ow * 4 + kx, ci]

    def test_mask_round_trip(self):
        gen = t.Generator().manual_seed(1)
        pos = t.randint(0, 2, (1000, 32), generator=gen).bool()
        pos[0], pos[1] = True, False
        pos[2] = False
        pos[2, 31] = True
        words = pack_mask(pos)
        assert words.dtype == t.int32 and words.shape == (1000,)
        assert words[0] == -1 and words[1] == 0 and words[2] == -2 ** 31
        assert t.equal(unpack_mask(words), pos)
        assert t.equal(pack_mask(unpack_mask(words)), words)
        for c in range(32):
            one = t.zeros(1, 32, dtype=t.bool)
            one[0, c] = True
            assert int(pack_mask(one)[0]) & 0xFFFFFFFF == 1 << c

    def test_round_bf16(self):
        x = t.tensor([256.0, 257.0, 258.0, 259.0, 261.0, -257.0, -259.0,
                      0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 18561.0],
                     dtype=t.float64)
        even = t.tensor([256.0, 256.0, 258.0, 260.0, 260.0, -256.0, -260.0,
                         0.0, 1.0, 1.0 + 2.0 ** -6, 18560.0],
                        dtype=t.float64)
        away = t.tensor([256.0, 258.0, 258.0, 260.0, 262.0, -258.0, -260.0,
                         0.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, 18560.0],
                        dtype=t.float64)
        assert t.equal(round_bf16(x), even)
        assert t.equal(round_bf16(x, ties_away=True), away)
        assert is_bf16_tie(x).tolist() == [False, True, False, True, True,
                                           True, True, False, True, True,
                                           False]
        # agrees with torch on float32 values (one rounding there too)
        y = t.randn(10000, generator=t.Generator().manual_seed(2))
        assert t.equal(round_bf16(y.double()), y.to(t.bfloat16).double())

    def test_cases_are_cached(self):
        assert forward_case(3, "signs", 1.0) is forward_case(3, "signs", 1.0)
        assert forward_reference(3, "signs", 1.0) \
            is forward_reference(3, "signs", 1.0, True)
        assert wrw_reference(1, "int", 1.0) is wrw_reference(1, "int", 1.0,
                                                             "none")


class TestReferencesAgainstAutograd:
    @pytest.mark.parametrize("kind,scale", [("dense", 1.0),
                                            ("dense", 2.0 ** -8),
                                            ("round", ROUND_SCALE)])
    def test_forward(self, kind, scale):
        case = forward_case(3, kind, scale)
        ref = forward_reference(3, kind, scale, True)
        x = dequant(case.frames, scale).double().permute(0, 3, 1, 2)
        w = case.weight.to(t.bfloat16).double()
        want = rows(F.conv2d(x, w, case.bias.double(), stride=4))
        assert t.allclose(ref.pre, want, rtol=1e-13, atol=1e-13)
        if kind == "dense":
            assert t.equal(ref.pre, want)
        # the explicit im2col GEMM on the repacked weight is the same op
        gemm = im2col(x.permute(0, 2, 3, 1)) @ repack(w) + case.bias.double()
        assert t.allclose(ref.pre, gemm, rtol=1e-13, atol=1e-13)
        assert t.equal(ref.y.double(), round_bf16(ref.pre))
        assert t.equal(ref.relu, t.relu(ref.y))
        assert t.equal(unpack_mask(ref.mask), ref.y > 0)

    def test_scaled_reference_is_the_scaled_case(self):
        for kind in ("taps5", "signs", "dense"):
            one = forward_reference(3, kind, 1.0)
            small = forward_reference(3, kind, 2.0 ** -8)
            assert t.equal(small.pre, one.pre * 2.0 ** -8)
            assert t.equal(small.y.double(), one.y.double() * 2.0 ** -8)
            assert t.equal(small.mask, one.mask)

    @pytest.mark.parametrize("mask_kind", ["none", "random", "from_forward"])
    @pytest.mark.parametrize("kind,scale", [("int", 1.0), ("int", 2.0 ** -8),
                                            ("round", ROUND_SCALE)])
    def test_weight_gradient(self, kind, scale, mask_kind):
        case = wrw_case(3, kind, scale)
        ref = wrw_reference(3, kind, scale, mask_kind)
        mask = wrw_mask(3, mask_kind)
        x = dequant(case.frames, scale).double().permute(0, 3, 1, 2)
        w = t.zeros(32, 4, 8, 8, dtype=t.float64, requires_grad=True)
        b = t.zeros(32, dtype=t.float64, requires_grad=True)
        y = F.conv2d(x, w, b, stride=4)
        d = case.dy.double()
        if mask is not None:
            d = d * unpack_mask(mask).double()
        y.backward(d.view(3, 20, 20, 32).permute(0, 3, 1, 2))
        assert t.allclose(ref.grad_w, w.grad, rtol=1e-13, atol=1e-13)
        assert t.allclose(ref.grad_b, b.grad, rtol=1e-13, atol=1e-13)
        if kind == "int":
            assert t.equal(ref.grad_w, w.grad)
            assert t.equal(ref.grad_b, b.grad)


class TestExactForwardConditions:
    @BOTH
    @SCALES
    @EXACT
    def test_sums_below_2_24_and_outputs(self, batch, kind, scale,
                                         with_bias):
        case = forward_case(batch, kind, scale)
        ref = forward_reference(batch, kind, scale, with_bias)
        # operands exact: integers (times the power-of-two scale)
        assert t.equal(case.weight, case.weight.round())
        assert t.equal(case.weight.to(t.bfloat16).float(), case.weight)
        assert t.equal(case.bias / scale, (case.bias / scale).round())
        # every partial sum is a multiple of scale below 2^24 * scale
        assert float(ref.s.max()) < 2 ** 24 * scale
        assert t.equal(ref.pre / scale, (ref.pre / scale).round())
        assert ref.y.shape == (batch * 400, 32)
        if kind != "dense":
            assert float(ref.pre.abs().max()) <= 256 * scale
            assert t.equal(ref.y.double(), ref.pre)  # exact in bf16

    @SCALES
    def test_taps_cover_every_tap_and_return_the_pixel(self, scale):
        seen = t.zeros(256, dtype=t.bool)
        frames = forward_case(3, "taps0", scale).frames
        cols = im2col(frames)
        for s, kind in enumerate(TAPS_KINDS):
            case = forward_case(3, kind, scale)
            assert case.frames is frames or t.equal(case.frames, frames)
            w_rs = repack(case.weight)
            assert t.equal(w_rs.sum(dim=0), t.ones(32))
            assert int((w_rs != 0).sum()) == 32
            for c in range(32):
                assert w_rs[s * 32 + c, c] == 1
                seen[s * 32 + c] = True
            ref = forward_reference(3, kind, scale, True)
            pixel = cols[:, s * 32:(s + 1) * 32]
            assert t.equal(ref.pre, (pixel + case.bias.double() / scale)
                           * scale)
            assert float(ref.pre.min()) >= -1 * scale
            assert float(ref.pre.max()) <= 256 * scale
            assert set((case.bias / scale).tolist()) == {-1.0, 0.0, 1.0}
        assert bool(seen.all())

    @pytest.mark.parametrize("kind", ["taps0", "dense"])
    @BATCH
    def test_forced_bytes_in_every_frame(self, batch, kind):
        if kind == "taps0" and batch != 3:
            batch = 3
        frames = forward_case(batch, kind, 1.0).frames
        assert frames.dtype == t.uint8 and frames.shape == (batch, 84, 84, 4)
        for b in range(batch):
            present = set(frames[b].unique().tolist())
            if kind == "taps0":
                assert set(FORCED_BYTES) <= present
            assert len(present) == 256   # full range

    @BOTH
    @SCALES
    @BATCH
    def test_signs_has_zeros_and_both_signs(self, batch, scale, with_bias):
        case = forward_case(batch, "signs", scale)
        assert set(case.frames.unique().tolist()) == {0, 1}
        assert set(case.weight.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert set((case.bias / scale).tolist()) <= {-2., -1., 0., 1., 2.}
        ref = forward_reference(batch, "signs", scale, with_bias)
        y = ref.y.double()
        zero = float((y == 0).double().mean())
        positive = float((y > 0).double().mean())
        print(f"signs B={batch} scale={scale} bias={with_bias}: max|y| "
              f"{float(y.abs().max()) / scale:.0f}, zero {zero:.3f}, "
              f"positive {positive:.3f}")
        assert float(y.abs().max()) <= 256 * scale
        assert zero > 0.01
        assert 0.2 < positive < 0.8
        # the mask differs between `> 0` and `>= 0`
        assert not t.equal(ref.mask, pack_mask(ref.y >= 0))

    @BOTH
    @SCALES
    @BATCH
    def test_dense_rounds_and_has_exact_ties(self, batch, scale, with_bias):
        ref = forward_reference(batch, "dense", scale, with_bias)
        ties = is_bf16_tie(ref.pre)
        inexact = ref.y.double() != ref.pre
        print(f"dense B={batch} scale={scale} bias={with_bias}: max|acc| "
              f"{float(ref.pre.abs().max()) / scale:.0f}, exact in bf16 "
              f"{1 - float(inexact.double().mean()):.3f}, ties "
              f"{int(ties.sum())}")
        assert int(ties.sum()) > 0
        assert float(inexact.double().mean()) > 0.5
        # ties go to even: half of them up, half down, none away only
        up = (ref.y.double().abs() > ref.pre.abs())[ties]
        assert bool(up.any()) and bool((~up).any())


class TestExactWeightGradientConditions:
    @pytest.mark.parametrize("mask_kind", MASK_KINDS)
    @SCALES
    @BATCH
    def test_sums_below_2_24(self, batch, scale, mask_kind):
        case = wrw_case(batch, "int", scale)
        assert case.dy.dtype == t.bfloat16
        assert set(case.dy.double().unique().tolist()) == {-2., -1., 0.,
                                                           1., 2.}
        assert len(case.frames.unique()) == 256
        ref = wrw_reference(batch, "int", scale, mask_kind)
        limit = 5 * 400 * 255 * 2
        assert limit < 2 ** 24
        assert float(ref.s_w.max()) <= limit * scale
        assert float(ref.s_b.max()) <= 5 * 400 * 2
        assert t.equal(ref.grad_w / scale, (ref.grad_w / scale).round())
        assert t.equal(ref.grad_b, ref.grad_b.round())
        if mask_kind == "clear":
            assert not ref.grad_w.any() and not ref.grad_b.any()
        else:
            assert ref.grad_w.abs().min() >= 0 and ref.grad_w.any()
        if mask_kind == "set":
            none = wrw_reference(batch, "int", scale, "none")
            assert t.equal(ref.grad_w, none.grad_w)
            assert t.equal(ref.grad_b, none.grad_b)

    @BATCH
    def test_masks(self, batch):
        K = batch * 400
        assert wrw_mask(batch, "none") is None
        for kind in MASK_KINDS[1:]:
            m = wrw_mask(batch, kind)
            assert m.dtype == t.int32 and m.shape == (K,)
        assert not wrw_mask(batch, "clear").any()
        assert bool(unpack_mask(wrw_mask(batch, "set")).all())
        frac = float(unpack_mask(wrw_mask(batch, "random")).double().mean())
        assert 0.45 < frac < 0.55
        fwd = forward_reference(batch, "signs", 1.0, True)
        assert t.equal(unpack_mask(wrw_mask(batch, "from_forward")),
                       fwd.y > 0)


class TestRoundingKind:
    @BATCH
    def test_bounds(self, batch):
        case = forward_case(batch, "round", ROUND_SCALE)
        assert t.equal(case.weight.to(t.bfloat16).float(), case.weight)
        ref = forward_reference(batch, "round", ROUND_SCALE, True)
        # F (K + 8) 2^-24 S + 2^-8 |ref| with F = 4, K = 256
        want = 4 * 264 * 2.0 ** -24 * ref.s + 2.0 ** -8 * ref.pre.abs()
        assert t.equal(ref.bound, want)
        assert bool((ref.s >= ref.pre.abs()).all())
        # the float64 value rounded to bf16 is itself inside the bound
        assert worst_ratio(ref.y, ref.pre, ref.bound) <= 1.0
        wref = wrw_reference(batch, "round", ROUND_SCALE, "random")
        k = 400 * batch + 8
        assert t.equal(wref.bound_w, 4 * k * 2.0 ** -24 * wref.s_w)
        assert t.equal(wref.bound_b, k * 2.0 ** -24 * wref.s_b)
        # well below the 2e-2 of max|ref| that the older tests allow
        assert float(wref.bound_w.max() / wref.grad_w.abs().max()) < 5e-3
        assert float(ref.bound.max() / ref.pre.abs().max()) < 5e-3

    def test_f_follows_from_the_probe_measurement(self):
        """2 for a truncating adder, or the next power of two above what
        one MFMA instruction showed on the device."""
        assert F_MFMA == max(2, 2 ** math.ceil(math.log2(
            MFMA_PROBE_MEASURED)))
        assert F_MFMA == 4

    def test_probe_tiles(self):
        a, b = probe_tiles()
        assert a.shape == (64, 16, 32) and b.shape == (64, 32, 16)
        assert a.dtype == b.dtype == t.bfloat16
        assert bool(t.isfinite(a.float()).all())
        assert bool(t.isfinite(b.float()).all())


# ---------------------------------------------------------------------
# Teeth: a float64 model of the kernels, wrong in one small way
# ---------------------------------------------------------------------
def model_forward(case, drop=None, swap=None, ties_away=False,
                  mask_ge=False, border=False):
    """The forward as an im2col GEMM in float64, optionally wrong:
    ``drop`` zeroes one tap, ``swap`` exchanges two, ``ties_away`` rounds
    the epilogue's ties away from zero, ``mask_ge`` sets the mask bit on
    ``y >= 0``, ``border`` reads the patches of output row 19 one image
    row too high. Returns (y bf16, relu bf16, mask)."""
    cols = model_cols(case.frames, case.scale, border)
    if drop is not None:
        cols[:, drop] = 0
    if swap is not None:
        cols[:, list(swap)] = cols[:, list(swap)[::-1]]
    pre = cols @ repack(case.weight).double() + case.bias.double()
    y = round_bf16(pre, ties_away).to(t.bfloat16)
    return y, t.relu(y), pack_mask(y >= 0 if mask_ge else y > 0)


def model_cols(frames, scale, border=False):
    x = dequant(frames, scale).double()
    cols = im2col(x).clone()
    if border:
        up = im2col(t.roll(x, 1, dims=1)).view(-1, 20, 20, 256)
        cols.view(-1, 20, 20, 256)[:, 19] = up[:, 19]
    return cols


def model_wrw(case, mask, border=False, drop=None):
    cols = model_cols(case.frames, case.scale, border)
    if drop is not None:
        cols[:, drop] = 0
    d = case.dy.double()
    if mask is not None:
        d = d * unpack_mask(mask).double()
    gw = (d.t() @ cols).view(32, 8, 8, 4).permute(0, 3, 1, 2)
    return gw, d.sum(dim=0)


def same(model, ref):
    y, relu, mask = model
    return (t.equal(y, ref.y) and t.equal(relu, ref.relu)
            and t.equal(mask, ref.mask))


class TestTeeth:
    KINDS = ("taps3", "signs", "dense")

    @SCALES
    @pytest.mark.parametrize("kind", KINDS)
    def test_the_unperturbed_model_is_the_reference(self, kind, scale):
        case = forward_case(3, kind, scale)
        assert same(model_forward(case), forward_reference(3, kind, scale))

    @SCALES
    @pytest.mark.parametrize("kind", KINDS)
    def test_one_dropped_tap(self, kind, scale):
        case = forward_case(3, kind, scale)
        ref = forward_reference(3, kind, scale)
        # taps3 holds taps 96..127
        for n in (96, 127, 101):
            assert not t.equal(model_forward(case, drop=n)[0], ref.y)

    def test_a_dropped_tap_is_seen_by_exactly_its_taps_set(self):
        for n in (0, 37, 255):
            for s, kind in enumerate(FWD_EXACT_KINDS[:8]):
                case = forward_case(3, kind, 1.0)
                ref = forward_reference(3, kind, 1.0)
                hit = not t.equal(model_forward(case, drop=n)[0], ref.y)
                assert hit == (n // 32 == s)

    @SCALES
    @pytest.mark.parametrize("kind", KINDS)
    def test_two_swapped_taps(self, kind, scale):
        case = forward_case(3, kind, scale)
        ref = forward_reference(3, kind, scale)
        # neighbours in ci, in kx and in ky, inside taps3's range
        for pair in ((96, 97), (100, 104), (96, 127), (97, 98)):
            got = model_forward(case, swap=pair)[0]
            if kind == "signs" and bool(
                    (repack(case.weight)[pair[0]]
                     == repack(case.weight)[pair[1]]).all()):
                continue
            assert not t.equal(got, ref.y), pair
        # a swap across taps sets: seen by both sets
        for kind2 in ("taps0", "taps7"):
            c = forward_case(3, kind2, scale)
            r = forward_reference(3, kind2, scale)
            assert not t.equal(model_forward(c, swap=(3, 250))[0], r.y)

    @BOTH
    @SCALES
    @BATCH
    def test_ties_rounded_away_from_zero(self, batch, scale, with_bias):
        case = forward_case(batch, "dense", scale)
        ref = forward_reference(batch, "dense", scale, with_bias)
        away = round_bf16(ref.pre, ties_away=True).to(t.bfloat16)
        differ = away != ref.y
        assert bool(differ.any())
        # and only at ties
        assert bool(is_bf16_tie(ref.pre)[differ].all())
        if with_bias:
            assert not t.equal(model_forward(case, ties_away=True)[0], ref.y)

    @SCALES
    @BATCH
    def test_mask_bit_set_on_zero(self, batch, scale):
        case = forward_case(batch, "signs", scale)
        ref = forward_reference(batch, "signs", scale)
        y, relu, mask = model_forward(case, mask_ge=True)
        assert t.equal(y, ref.y) and t.equal(relu, ref.relu)
        assert not t.equal(mask, ref.mask)
        # and the weight gradient masked by it differs too
        wcase = wrw_case(batch, "int", scale)
        good = model_wrw(wcase, ref.mask)
        bad = model_wrw(wcase, mask)
        assert not t.equal(good[0], bad[0])
        assert not t.equal(good[1], bad[1])

    @SCALES
    @pytest.mark.parametrize("kind", KINDS)
    def test_border_row_from_the_neighbouring_row(self, kind, scale):
        case = forward_case(3, kind, scale)
        ref = forward_reference(3, kind, scale)
        got = model_forward(case, border=True)[0]
        assert not t.equal(got, ref.y)
        rows_hit = (got != ref.y).any(dim=1).view(3, 20, 20)
        assert not rows_hit[:, :19].any()      # only output row 19
        assert bool(rows_hit[:, 19].any(dim=1).all())   # in every frame

    @pytest.mark.parametrize("mask_kind", ["none", "random", "set",
                                           "from_forward"])
    @SCALES
    @BATCH
    def test_weight_gradient_perturbations(self, batch, scale, mask_kind):
        case = wrw_case(batch, "int", scale)
        mask = wrw_mask(batch, mask_kind)
        ref = wrw_reference(batch, "int", scale, mask_kind)
        gw, gb = model_wrw(case, mask)
        assert t.equal(gw, ref.grad_w) and t.equal(gb, ref.grad_b)
        assert not t.equal(model_wrw(case, mask, border=True)[0],
                           ref.grad_w)
        assert not t.equal(model_wrw(case, mask, drop=77)[0], ref.grad_w)
        # one dy element lost (a chunk tail, a frame edge)
        d = case.dy.clone()
        nz = int(d[-1].double().abs().argmax())
        assert d[-1, nz] != 0
        if mask is not None and not bool(unpack_mask(mask)[-1, nz]):
            return
        d[-1, nz] = 0
        lost = wrw_float64(case.frames, d, mask, scale)
        assert not t.equal(lost[0], ref.grad_w)
        assert not t.equal(lost[1], ref.grad_b)
