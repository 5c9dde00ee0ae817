"""Frame-resident (v4) stem kernels against the v3 kernels they replace.

The v4 forward keeps a whole frame in LDS and walks the batch with
persistent workgroups. It must return the same bits as v3, output and
sign mask, because the fused model is compared bit for bit with the
unfused composition elsewhere in the suite. The shapes are the smallest
at which the frame loop can go wrong: one frame, fewer frames than
workgroups, a grid forced to 2 so that the loop wraps with unequal trip
counts and the prefetch hits its tail, and a grid larger than the batch.

The v4 weight gradient sums the same products in another order (fp32
MFMA accumulation per workgroup, then fp32 atomics), so it is held to
the project's bound for two orders of one fp32 sum against v3, and to
the bf16 bound against a float64 reference built from the bf16-rounded
operands. Batch 1, 3 and 5 at 1, 2 and 2048 workgroups: one workgroup
walking several frames, an uneven split, and more workgroups than
frames.
"""
import pytest
import torch as t
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = "cuda:0"
SCALE = 1.0 / 255.0
FRAME_BYTES = 84 * 84 * 4

# two evaluations of one fp32 sum in different orders (ATOMIC_RTOL of
# tests/test_fused_act_gpu.py), relative to max|ref|
ATOMIC_RTOL = 1e-5
# bf16 operands against a float64 reference (tests/test_fused_conv_gpu.py)
BF16_RTOL = 2e-2

# (batch, MACHIN_CONV1_FWD_WG or None)
CASES = [(1, None), (3, None), (5, 2), (2, 4)]


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
    return b, w_rs


def _unpack_mask(mask):
    """[K] int32 words -> [K, 32] bool, bit c of word k at [k, c]."""
    shifts = t.arange(32, device=mask.device, dtype=t.int32)
    return ((mask.view(-1, 1) >> shifts) & 1).bool()


def _bias(b, with_bias):
    return b if with_bias else t.empty(0, device=DEV)


_V3 = {}


def _v3_reference(monkeypatch, batch, with_bias):
    """(frames, plain, relu, mask) of the v3 kernels, computed once per
    (batch, with_bias) and never modified."""
    key = (batch, with_bias)
    if key not in _V3:
        ext = _ext()
        frames = _frames_nhwc(batch, 40 + batch)
        b, w_rs = _stem_weights(3)
        monkeypatch.setenv("MACHIN_CONV1_V", "3")
        plain = ext.conv1_fwd(frames, w_rs, _bias(b, with_bias), SCALE)
        y, mask = ext.conv1_fwd_relu(frames, w_rs, _bias(b, with_bias),
                                     SCALE)
        t.cuda.synchronize()
        _V3[key] = (frames, plain, y, mask)
    return _V3[key]


def _select_v4(monkeypatch, fwd_wg):
    monkeypatch.setenv("MACHIN_CONV1_V", "4")
    if fwd_wg is None:
        monkeypatch.delenv("MACHIN_CONV1_FWD_WG", raising=False)
    else:
        monkeypatch.setenv("MACHIN_CONV1_FWD_WG", str(fwd_wg))


class TestFrameResidentForward:
    @pytest.mark.parametrize("with_bias", [True, False])
    @pytest.mark.parametrize("batch,fwd_wg", CASES)
    def test_bit_identical_to_v3(self, monkeypatch, batch, fwd_wg,
                                 with_bias):
        ext = _ext()
        frames, ref_plain, ref_y, ref_mask = _v3_reference(
            monkeypatch, batch, with_bias
        )
        b, w_rs = _stem_weights(3)
        bias = _bias(b, with_bias)
        _select_v4(monkeypatch, fwd_wg)
        plain = ext.conv1_fwd(frames, w_rs, bias, SCALE)
        y, mask = ext.conv1_fwd_relu(frames, w_rs, bias, SCALE)
        assert plain.shape == (batch * 400, 32)
        assert plain.dtype == t.bfloat16
        assert mask.shape == (batch * 400,) and mask.dtype == t.int32
        assert t.equal(plain, ref_plain)
        assert t.equal(y, ref_y)
        assert t.equal(mask, ref_mask)
        assert t.equal(y, t.relu(plain))
        assert t.equal(_unpack_mask(mask), y > 0)
        # both signs must occur for the checks above to mean anything
        frac = (y > 0).float().mean().item()
        assert 0.2 < frac < 0.8, frac
        # a second call on the same input: a stale LDS frame would show
        plain2 = ext.conv1_fwd(frames, w_rs, bias, SCALE)
        y2, mask2 = ext.conv1_fwd_relu(frames, w_rs, bias, SCALE)
        assert t.equal(plain2, plain)
        assert t.equal(y2, y)
        assert t.equal(mask2, mask)

    @pytest.mark.parametrize("batch", [1, 3])
    def test_unaligned_frames_take_the_v3_kernels(self, monkeypatch,
                                                  batch):
        # a contiguous view that starts 1 byte into a larger buffer: the
        # 16-byte loads of v4 do not apply, the launcher runs v3
        ext = _ext()
        frames, ref_plain, ref_y, ref_mask = _v3_reference(
            monkeypatch, batch, True
        )
        b, w_rs = _stem_weights(3)
        buf = t.zeros(batch * FRAME_BYTES + 16, dtype=t.uint8, device=DEV)
        shifted = buf[1:1 + batch * FRAME_BYTES].view(batch, 84, 84, 4)
        shifted.copy_(frames)
        assert shifted.is_contiguous()
        assert shifted.data_ptr() % 16 == 1
        _select_v4(monkeypatch, None)
        plain = ext.conv1_fwd(shifted, w_rs, b, SCALE)
        y, mask = ext.conv1_fwd_relu(shifted, w_rs, b, SCALE)
        assert t.equal(plain, ref_plain)
        assert t.equal(y, ref_y)
        assert t.equal(mask, ref_mask)

    def test_version_4_is_the_default(self, monkeypatch):
        ext = _ext()
        frames, ref_plain, ref_y, ref_mask = _v3_reference(
            monkeypatch, 3, True
        )
        b, w_rs = _stem_weights(3)
        monkeypatch.delenv("MACHIN_CONV1_V", raising=False)
        monkeypatch.delenv("MACHIN_CONV1_FWD_WG", raising=False)
        y, mask = ext.conv1_fwd_relu(frames, w_rs, b, SCALE)
        assert t.equal(ext.conv1_fwd(frames, w_rs, b, SCALE), ref_plain)
        assert t.equal(y, ref_y)
        assert t.equal(mask, ref_mask)


def _wrw_inputs(batch, kind):
    """(frames, dy, mask or None): kind is none / random / clear / set."""
    K = batch * 400
    frames = _frames_nhwc(batch, 60 + batch)
    g = t.Generator(device=DEV).manual_seed(7 + batch)
    dy = (t.randn(K, 32, device=DEV, generator=g) * 0.1).to(t.bfloat16)
    if kind == "none":
        mask = None
    elif kind == "random":
        mask = t.randint(-2 ** 31, 2 ** 31, (K,), device=DEV,
                         generator=g, dtype=t.int64).to(t.int32)
    elif kind == "clear":
        mask = t.zeros(K, dtype=t.int32, device=DEV)
    else:
        mask = t.full((K,), -1, dtype=t.int32, device=DEV)
    return frames, dy, mask


def _wrw_call(frames, dy, mask):
    ext = _ext()
    if mask is None:
        return ext.conv1_wrw(dy, frames, SCALE)
    return ext.conv1_wrw_masked(dy, mask, frames, SCALE)


def _wrw_float64(frames, dy, mask):
    """dW, db in float64 from the operands the kernels multiply:
    bf16(u8 * scale) and the masked bf16 dy."""
    batch = frames.shape[0]
    x = (frames.float() * SCALE).to(t.bfloat16).double()
    cols = F.unfold(x.permute(0, 3, 1, 2), 8, stride=4)  # [B, 256, 400]
    d = dy.double()
    if mask is not None:
        d = d * _unpack_mask(mask).double()
    d = d.view(batch, 400, 32)
    gw = t.einsum("bpo,bnp->on", d, cols).view(32, 4, 8, 8)
    return gw, d.sum(dim=(0, 1))


_WRW = {}


def _wrw_reference(monkeypatch, batch, kind):
    """Inputs, float64 reference and v3 results at 1, 2 and 2048
    workgroups, computed once per (batch, kind)."""
    key = (batch, kind)
    if key not in _WRW:
        frames, dy, mask = _wrw_inputs(batch, kind)
        monkeypatch.setenv("MACHIN_CONV1_V", "3")
        v3 = {}
        for wg in (1, 2, 2048):
            monkeypatch.setenv("MACHIN_CONV1_WG", str(wg))
            v3[wg] = _wrw_call(frames, dy, mask)
        t.cuda.synchronize()
        _WRW[key] = (frames, dy, mask, _wrw_float64(frames, dy, mask), v3)
    return _WRW[key]


def _max_diff(a, b):
    return (a.double() - b.double()).abs().max().item()


class TestFrameResidentWeightGrad:
    @pytest.mark.parametrize("kind", ["none", "random", "clear", "set"])
    @pytest.mark.parametrize("wg", [1, 2, 2048])
    @pytest.mark.parametrize("batch", [1, 3, 5])
    def test_against_v3_and_float64(self, monkeypatch, batch, wg, kind):
        frames, dy, mask, (ref_w, ref_b), v3 = _wrw_reference(
            monkeypatch, batch, kind
        )
        monkeypatch.setenv("MACHIN_CONV1_V", "4")
        monkeypatch.setenv("MACHIN_CONV1_WG", str(wg))
        gw, gb = _wrw_call(frames, dy, mask)
        assert gw.shape == (32, 4, 8, 8) and gw.dtype == t.float32
        assert gb.shape == (32,) and gb.dtype == t.float32
        if kind == "clear":
            assert t.equal(gw, t.zeros_like(gw))
            assert t.equal(gb, t.zeros_like(gb))
            return
        tag = f"B={batch} wg={wg} {kind}"
        for name, got, ref64, ref3 in (
            ("grad_w", gw, ref_w, [r[0] for r in (v3[1], v3[2], v3[2048])]),
            ("grad_b", gb, ref_b, [r[1] for r in (v3[1], v3[2], v3[2048])]),
        ):
            scale = ref64.abs().max().item()
            bound = ATOMIC_RTOL * scale
            # the reference against itself under another order
            spread = _max_diff(ref3[0], ref3[2])
            same_wg = ref3[(1, 2, 2048).index(wg)]
            diff = _max_diff(got, same_wg)
            rel64 = _max_diff(got, ref64) / max(scale, 1e-3)
            print(f"{name} {tag}: v3 wg=1 vs wg=2048 {spread:.3e}, "
                  f"v4 vs v3 {diff:.3e}, bound {bound:.3e}, "
                  f"v4 vs float64 rel {rel64:.3e}")
            assert diff <= bound, f"{name} {tag}: {diff} > {bound}"
            assert rel64 < BF16_RTOL, f"{name} {tag}: rel {rel64}"

    @pytest.mark.parametrize("wg", [1, 2, 2048])
    @pytest.mark.parametrize("batch", [1, 3, 5])
    def test_all_set_mask_equals_unmasked(self, monkeypatch, batch, wg):
        frames, dy, _ = _wrw_inputs(batch, "none")
        mask = t.full((batch * 400,), -1, dtype=t.int32, device=DEV)
        monkeypatch.setenv("MACHIN_CONV1_V", "4")
        monkeypatch.setenv("MACHIN_CONV1_WG", str(wg))
        gw, gb = _wrw_call(frames, dy, None)
        mw, mb = _wrw_call(frames, dy, mask)
        for name, got, ref in (("grad_w", mw, gw), ("grad_b", mb, gb)):
            bound = ATOMIC_RTOL * ref.abs().max().item()
            diff = _max_diff(got, ref)
            print(f"{name} B={batch} wg={wg}: masked(all set) vs "
                  f"unmasked {diff:.3e}, bound {bound:.3e}")
            assert diff <= bound, f"{name}: {diff} > {bound}"

    def test_unaligned_frames_take_the_v3_kernels(self, monkeypatch):
        frames, dy, mask, _, v3 = _wrw_reference(monkeypatch, 3, "random")
        buf = t.zeros(3 * FRAME_BYTES + 16, dtype=t.uint8, device=DEV)
        shifted = buf[1:1 + 3 * FRAME_BYTES].view(3, 84, 84, 4)
        shifted.copy_(frames)
        monkeypatch.setenv("MACHIN_CONV1_V", "4")
        monkeypatch.setenv("MACHIN_CONV1_WG", "2048")
        gw, gb = _wrw_call(shifted, dy, mask)
        bound = ATOMIC_RTOL * v3[2048][0].abs().max().item()
        assert _max_diff(gw, v3[2048][0]) <= bound
