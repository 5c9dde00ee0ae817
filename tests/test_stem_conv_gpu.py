"""Every generation of the stem conv kernels
(``machin_amd/ops/hip/conv1_wrw.hip``, ``MACHIN_CONV1_V`` = 1..4) against
the float64 references of ``util_stem_conv``.

1. Exact: on the integer kinds every product and partial sum is exact
   in fp32 in any order, so the output, the ReLU output, the mask word
   and both gradients must equal the reference bit for bit, whatever the
   kernel version, the grid or the split-K geometry. A dropped or
   swapped tap, a wrong byte lane, position or channel, a tie rounded
   the wrong way or a mask bit set on ``y == 0`` cannot hide
   (``test_stem_conv_cpu.py`` shows that on the references).
2. Rounding: on random inputs at scale 1/255,
   ``|got - ref| <= F (K + 8) 2^-24 S (+ 2^-8 |ref|)`` per element, with
   ``F`` derived in ``util_stem_conv`` and confirmed here on one MFMA
   instruction, never on the conv kernels.
3. The module: ``FusedAtariConv1`` on integer weights equals the float64
   conv autograd bit for bit (repack, layout permutes, reorder kernel).
4. The bindings reject what the kernels cannot take.
"""
import functools
from types import SimpleNamespace

import pytest
import torch as t

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from util_stem_conv import (  # noqa: E402
    BATCHES, EXACT_SCALES, F_MFMA, FWD_EXACT_KINDS, MASK_KINDS, ROUND_SCALE,
    forward_case, forward_reference, probe_tiles, repack, unpack_mask,
    worst_ratio, wrw_case, wrw_float64, wrw_mask, wrw_reference,
)

DEV = "cuda:0"
FRAME_BYTES = 84 * 84 * 4
TAPS_KINDS = FWD_EXACT_KINDS[:8]

# (MACHIN_CONV1_V, MACHIN_CONV1_FWD_WG or None). The grid override only
# exists in v4: 2 makes the frame loop wrap with unequal trip counts at
# batch 3 and 5, 4 leaves workgroups idle at batch 1 and 3
FWD_CONFIGS = [("1", None), ("2", None), ("3", None), ("4", None),
               ("4", "2"), ("4", "4")]
# conv1_fwd_relu has the v3 and v4 kernels only
RELU_CONFIGS = [c for c in FWD_CONFIGS if c[0] in ("3", "4")]
WGS = ("1", "2", "2048")


def config_id(c):
    return f"v{c[0]}" + (f"-grid{c[1]}" if c[1] else "")


def _ext():
    from machin_amd.ops import _require_ext

    return _require_ext()


def select(monkeypatch, version, fwd_wg=None, wg=None):
    monkeypatch.setenv("MACHIN_CONV1_V", version)
    for name, value in (("MACHIN_CONV1_FWD_WG", fwd_wg),
                        ("MACHIN_CONV1_WG", wg)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def shifted(frames):
    """The same frames, contiguous, 1 byte into a larger buffer: the
    16-byte loads of v4 do not apply and its launchers run v3."""
    n = frames.numel()
    buf = t.zeros(n + 16, dtype=t.uint8, device=frames.device)
    out = buf[1:1 + n].view(frames.shape)
    out.copy_(frames)
    assert out.is_contiguous() and out.data_ptr() % 16 == 1
    return out


@functools.lru_cache(maxsize=None)
def fwd_inputs(batch, kind, scale):
    """Device copies of a forward case, shared and never modified."""
    case = forward_case(batch, kind, scale)
    return SimpleNamespace(
        frames=case.frames.to(DEV),
        w_rs=repack(case.weight).to(t.bfloat16).contiguous().to(DEV),
        bias=case.bias.to(DEV), empty=t.empty(0, device=DEV),
        scale=scale,
    )


@functools.lru_cache(maxsize=None)
def fwd_expected(batch, kind, scale, with_bias):
    ref = forward_reference(batch, kind, scale, with_bias)
    return SimpleNamespace(y=ref.y.to(DEV), relu=ref.relu.to(DEV),
                           mask=ref.mask.to(DEV))


@functools.lru_cache(maxsize=None)
def wrw_inputs(batch, kind, scale, mask_kind):
    case = wrw_case(batch, kind, scale)
    mask = wrw_mask(batch, mask_kind)
    return SimpleNamespace(
        frames=case.frames.to(DEV), dy=case.dy.to(DEV),
        mask=None if mask is None else mask.to(DEV), scale=scale,
    )


def wrw_call(inp, frames=None):
    ext = _ext()
    frames = inp.frames if frames is None else frames
    if inp.mask is None:
        return ext.conv1_wrw(inp.dy, frames, inp.scale)
    return ext.conv1_wrw_masked(inp.dy, inp.mask, frames, inp.scale)


def exact_cases():
    out = [(3, k) for k in TAPS_KINDS]
    return out + [(b, k) for b in BATCHES for k in ("signs", "dense")]


EXACT = pytest.mark.parametrize("batch,kind", exact_cases())


class TestForwardExact:
    def _run(self, monkeypatch, config, batch, kind, relu):
        ext = _ext()
        version, fwd_wg = config
        select(monkeypatch, version, fwd_wg)
        for scale in EXACT_SCALES:
            inp = fwd_inputs(batch, kind, scale)
            frames = [inp.frames]
            if config == ("4", None):
                frames.append(shifted(inp.frames))
            for with_bias in (True, False):
                want = fwd_expected(batch, kind, scale, with_bias)
                bias = inp.bias if with_bias else inp.empty
                tag = f"scale={scale} bias={with_bias}"
                # the second call on the same input: a stale LDS image
                # or an output that depends on what was there before
                for fr in frames + frames[:1]:
                    if relu:
                        y, mask = ext.conv1_fwd_relu(fr, inp.w_rs, bias,
                                                     scale)
                        assert mask.dtype == t.int32
                        assert mask.shape == (batch * 400,)
                        assert t.equal(y, want.relu), tag
                        assert t.equal(mask, want.mask), tag
                    else:
                        y = ext.conv1_fwd(fr, inp.w_rs, bias, scale)
                        assert t.equal(y, want.y), tag
                    assert y.dtype == t.bfloat16
                    assert y.shape == (batch * 400, 32)

    @EXACT
    @pytest.mark.parametrize("config", FWD_CONFIGS, ids=config_id)
    def test_conv1_fwd(self, monkeypatch, config, batch, kind):
        self._run(monkeypatch, config, batch, kind, relu=False)

    @EXACT
    @pytest.mark.parametrize("config", RELU_CONFIGS, ids=config_id)
    def test_conv1_fwd_relu(self, monkeypatch, config, batch, kind):
        self._run(monkeypatch, config, batch, kind, relu=True)


class TestWeightGradExact:
    def _run(self, monkeypatch, version, wg, batch, mask_kind):
        select(monkeypatch, version, wg=wg)
        for scale in EXACT_SCALES:
            inp = wrw_inputs(batch, "int", scale, mask_kind)
            ref = wrw_reference(batch, "int", scale, mask_kind)
            runs = [inp.frames]
            if version == "4":
                runs.append(shifted(inp.frames))
            for fr in runs:
                gw, gb = wrw_call(inp, fr)
                assert gw.shape == (32, 4, 8, 8) and gw.dtype == t.float32
                assert gb.shape == (32,) and gb.dtype == t.float32
                # atomics on integers are exact: no geometry changes a bit
                assert t.equal(gw.cpu().double(), ref.grad_w), scale
                assert t.equal(gb.cpu().double(), ref.grad_b), scale
                if mask_kind == "clear":
                    assert not gw.any() and not gb.any()

    @pytest.mark.parametrize("batch", BATCHES)
    @pytest.mark.parametrize("wg", WGS)
    @pytest.mark.parametrize("version", ["1", "2", "3", "4"])
    def test_conv1_wrw(self, monkeypatch, version, wg, batch):
        self._run(monkeypatch, version, wg, batch, "none")

    @pytest.mark.parametrize("mask_kind", MASK_KINDS[1:])
    @pytest.mark.parametrize("batch", BATCHES)
    @pytest.mark.parametrize("wg", WGS)
    @pytest.mark.parametrize("version", ["3", "4"])
    def test_conv1_wrw_masked(self, monkeypatch, version, wg, batch,
                              mask_kind):
        self._run(monkeypatch, version, wg, batch, mask_kind)


class TestRoundingBound:
    """Batch 1 and 3 of the same grid on the rounding kind."""

    def _forward(self, monkeypatch, config, batch, relu):
        ext = _ext()
        select(monkeypatch, *config)
        inp = fwd_inputs(batch, "round", ROUND_SCALE)
        for with_bias in (True, False):
            ref = forward_reference(batch, "round", ROUND_SCALE, with_bias)
            bias = inp.bias if with_bias else inp.empty
            name = "conv1_fwd_relu" if relu else "conv1_fwd"
            if relu:
                y, mask = ext.conv1_fwd_relu(inp.frames, inp.w_rs, bias,
                                             ROUND_SCALE)
                # the 1-Lipschitz ReLU keeps the bound; the mask is that
                # of the values the kernel stored
                ratio = worst_ratio(y, t.relu(ref.pre), ref.bound)
                assert t.equal(unpack_mask(mask), y > 0)
            else:
                y = ext.conv1_fwd(inp.frames, inp.w_rs, bias, ROUND_SCALE)
                ratio = worst_ratio(y, ref.pre, ref.bound)
            print(f"ROUNDING {name} {config_id(config)} B={batch} "
                  f"bias={with_bias}: worst |err| / bound = {ratio:.3f}")
            assert ratio <= 1.0

    @pytest.mark.parametrize("batch", [1, 3])
    @pytest.mark.parametrize("config", FWD_CONFIGS, ids=config_id)
    def test_conv1_fwd(self, monkeypatch, config, batch):
        self._forward(monkeypatch, config, batch, relu=False)

    @pytest.mark.parametrize("batch", [1, 3])
    @pytest.mark.parametrize("config", RELU_CONFIGS, ids=config_id)
    def test_conv1_fwd_relu(self, monkeypatch, config, batch):
        self._forward(monkeypatch, config, batch, relu=True)

    def _wrw(self, monkeypatch, version, wg, batch, mask_kind):
        select(monkeypatch, version, wg=wg)
        inp = wrw_inputs(batch, "round", ROUND_SCALE, mask_kind)
        ref = wrw_reference(batch, "round", ROUND_SCALE, mask_kind)
        gw, gb = wrw_call(inp)
        rw = worst_ratio(gw, ref.grad_w, ref.bound_w)
        rb = worst_ratio(gb, ref.grad_b, ref.bound_b)
        name = "conv1_wrw" if inp.mask is None else "conv1_wrw_masked"
        print(f"ROUNDING {name} v{version} wg={wg} B={batch} {mask_kind}: "
              f"worst |err| / bound = {rw:.2e} (grad_w) {rb:.2e} (grad_b)")
        assert rw <= 1.0
        assert rb <= 1.0

    @pytest.mark.parametrize("batch", [1, 3])
    @pytest.mark.parametrize("wg", WGS)
    @pytest.mark.parametrize("version", ["1", "2", "3", "4"])
    def test_conv1_wrw(self, monkeypatch, version, wg, batch):
        self._wrw(monkeypatch, version, wg, batch, "none")

    @pytest.mark.parametrize("mask_kind", MASK_KINDS[1:])
    @pytest.mark.parametrize("batch", [1, 3])
    @pytest.mark.parametrize("wg", WGS)
    @pytest.mark.parametrize("version", ["3", "4"])
    def test_conv1_wrw_masked(self, monkeypatch, version, wg, batch,
                              mask_kind):
        self._wrw(monkeypatch, version, wg, batch, mask_kind)


class TestMfmaProbe:
    def test_exact_on_integers(self):
        """Asymmetric small-integer A and B: one MFMA tile equals
        ``A @ B`` bit for bit (a row/column or k-slot swap cannot hide
        behind a tolerance)."""
        ext = _ext()
        gen = t.Generator().manual_seed(11)
        A = t.randint(-3, 4, (16, 32), generator=gen).double()
        B = t.randint(-4, 6, (32, 16), generator=gen).double()
        # make rows, columns and k-slots all distinguishable
        A += t.arange(16).double().view(16, 1) * 8
        B += t.arange(32).double().view(32, 1) % 5
        B += t.arange(16).double().view(1, 16) * 3
        ref = A @ B
        assert float((A.abs() @ B.abs()).max()) < 2 ** 24
        assert not t.equal(ref, ref.t())
        a16, b16 = A.to(t.bfloat16), B.to(t.bfloat16)
        assert t.equal(a16.double(), A) and t.equal(b16.double(), B)
        D = ext.mfma_probe(a16.to(DEV).contiguous(), b16.to(DEV).contiguous())
        assert D.dtype == t.float32 and D.shape == (16, 16)
        assert t.equal(D.cpu().double(), ref)

    def test_rounding_constant(self):
        """The ``F`` of the rounding bound on the instruction alone: one
        ``v_mfma_f32_16x16x32_bf16`` is off by at most
        ``F_MFMA * 2^-24 * S`` per element."""
        ext = _ext()
        A, B = probe_tiles()
        worst = 0.0
        for a, b in zip(A.to(DEV), B.to(DEV)):
            D = ext.mfma_probe(a.contiguous(), b.contiguous())
            ref = a.cpu().double() @ b.cpu().double()
            s = a.cpu().double().abs() @ b.cpu().double().abs()
            worst = max(worst, worst_ratio(D, ref, s * 2.0 ** -24))
        print(f"ROUNDING mfma_probe: worst |err| / (S * 2^-24) = "
              f"{worst:.3f} per instruction, F = {F_MFMA}")
        assert worst <= F_MFMA


class TestModuleExact:
    """``FusedAtariConv1(scale=1.0)`` with integer weights and bias
    against the float64 conv autograd: pins the weight repack, the
    NHWC/NCHW permutes of forward and backward and the reorder kernel's
    ``[32, 256] -> [32, 4, 8, 8]`` layout. With ``MACHIN_CONV1_V`` 1 or 2
    the module composes the plain kernels with ``torch.relu``."""

    @pytest.mark.parametrize("kind", ["signs", "dense"])
    @pytest.mark.parametrize("layout", ["channels_last", "nchw"])
    @pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
    @pytest.mark.parametrize("version", ["1", "2", "3", "4"])
    def test_bit_equal_to_float64_autograd(self, monkeypatch, version,
                                           relu, layout, kind):
        from machin_amd.ops.fused_conv import FusedAtariConv1

        batch = 3
        select(monkeypatch, version)
        case = forward_case(batch, kind, 1.0)
        ref = forward_reference(batch, kind, 1.0, True)
        dy = wrw_case(batch, "int", 1.0).dy          # integers -2..2
        mask = ref.mask if relu else None
        ref_w, ref_b, s_w, _ = wrw_float64(case.frames, dy, mask, 1.0)
        assert float(s_w.max()) < 2 ** 24

        stem = FusedAtariConv1(scale=1.0, relu=relu).to(DEV)
        with t.no_grad():
            stem.weight.copy_(case.weight)
            stem.bias.copy_(case.bias)
        frames = case.frames.to(DEV).permute(0, 3, 1, 2)   # channels-last
        gy = dy.to(DEV).view(batch, 20, 20, 32).permute(0, 3, 1, 2)
        if layout == "nchw":
            frames, gy = frames.contiguous(), gy.contiguous()
            assert frames.is_contiguous() and gy.is_contiguous()
        else:
            assert frames.is_contiguous(memory_format=t.channels_last)
        y = stem(frames)
        assert y.shape == (batch, 32, 20, 20) and y.dtype == t.bfloat16
        want = ref.relu if relu else ref.y
        assert t.equal(y.permute(0, 2, 3, 1).reshape(-1, 32).cpu(), want)
        y.backward(gy)
        assert stem.weight.grad.shape == (32, 4, 8, 8)
        assert t.equal(stem.weight.grad.cpu().double(), ref_w)
        assert t.equal(stem.bias.grad.cpu().double(), ref_b)


class TestBindingChecks:
    """Arguments the kernels would index out of bounds, or silently
    misread, stop in the bindings; an empty batch launches nothing."""

    def _good(self, batch=2):
        inp = fwd_inputs(3, "signs", 1.0)
        frames = inp.frames[:batch].contiguous()
        dy = t.ones(batch * 400, 32, dtype=t.bfloat16, device=DEV)
        mask = t.full((batch * 400,), -1, dtype=t.int32, device=DEV)
        return frames, inp.w_rs, inp.bias, dy, mask

    def _bad_frames(self):
        frames = self._good()[0]
        return {
            "nchw": frames.permute(0, 3, 1, 2).contiguous(),
            "smaller": frames[:, :80].contiguous(),
            "narrower": frames[:, :, :80].contiguous(),
            "3 channels": frames[..., :3].contiguous(),
            "3 dims": frames[0].contiguous(),
            "5 dims": frames.unsqueeze(0).contiguous(),
            "flat": frames.view(-1),
            "not contiguous": frames.permute(0, 2, 1, 3),
            "int8": frames.view(t.int8),
            "float": frames.float(),
            "cpu": frames.cpu(),
        }

    @pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
    def test_forward_rejects(self, relu):
        ext = _ext()
        fn = ext.conv1_fwd_relu if relu else ext.conv1_fwd
        frames, w_rs, bias, _, _ = self._good()
        fn(frames, w_rs, bias, 1.0)
        for what, bad in self._bad_frames().items():
            with pytest.raises(RuntimeError):
                fn(bad, w_rs, bias, 1.0)
                pytest.fail(f"frames {what} accepted")
        bad_weights = {
            "cpu": w_rs.cpu(), "fp32": w_rs.float(),
            "transposed": w_rs.t().contiguous(), "view": w_rs.t(),
            "flat": w_rs.view(-1), "short": w_rs[:128].contiguous(),
            "3 dims": w_rs.view(256, 32, 1),
        }
        for what, bad in bad_weights.items():
            with pytest.raises(RuntimeError):
                fn(frames, bad, bias, 1.0)
                pytest.fail(f"weight {what} accepted")
        bad_biases = {
            "cpu": bias.cpu(), "bf16": bias.to(t.bfloat16),
            "short": bias[:16].contiguous(), "long": bias.repeat(2),
            "2 dims": bias.view(1, 32), "strided": bias.repeat(2)[::2],
        }
        for what, bad in bad_biases.items():
            with pytest.raises(RuntimeError):
                fn(frames, w_rs, bad, 1.0)
                pytest.fail(f"bias {what} accepted")

    @pytest.mark.parametrize("masked", [False, True],
                             ids=["plain", "masked"])
    def test_weight_gradient_rejects(self, masked):
        ext = _ext()
        frames, _, _, dy, mask = self._good()

        def fn(dy, frames, mask=mask):
            if masked:
                return ext.conv1_wrw_masked(dy, mask, frames, 1.0)
            return ext.conv1_wrw(dy, frames, 1.0)

        fn(dy, frames)
        for what, bad in self._bad_frames().items():
            with pytest.raises(RuntimeError):
                fn(dy, bad)
                pytest.fail(f"frames {what} accepted")
        bad_dys = {
            "3 dims": dy.view(2, 400, 32), "4 dims": dy.view(2, 20, 20, 32),
            "1 dim": dy.view(-1), "short": dy[:400].contiguous(),
            "long": dy.repeat(2, 1), "16 columns": dy[:, :16].contiguous(),
            "strided": dy.repeat(1, 2)[:, ::2], "fp32": dy.float(),
            "cpu": dy.cpu(),
        }
        for what, bad in bad_dys.items():
            with pytest.raises(RuntimeError):
                fn(bad, frames)
                pytest.fail(f"dy {what} accepted")
        if not masked:
            return
        bad_masks = {
            "cpu": mask.cpu(), "int64": mask.long(),
            "short": mask[:400].contiguous(), "2 dims": mask.view(-1, 1),
            "strided": mask.repeat(2)[::2],
            "unaligned": mask.repeat(2)[1:801],
        }
        for what, bad in bad_masks.items():
            with pytest.raises(RuntimeError):
                fn(dy, frames, bad)
                pytest.fail(f"mask {what} accepted")

    @pytest.mark.parametrize("version", ["1", "2", "3", "4"])
    def test_empty_batch(self, monkeypatch, version):
        ext = _ext()
        select(monkeypatch, version)
        _, w_rs, bias, _, _ = self._good()
        frames = t.empty(0, 84, 84, 4, dtype=t.uint8, device=DEV)
        dy = t.empty(0, 32, dtype=t.bfloat16, device=DEV)
        mask = t.empty(0, dtype=t.int32, device=DEV)
        y = ext.conv1_fwd(frames, w_rs, bias, 1.0)
        assert y.shape == (0, 32) and y.dtype == t.bfloat16
        y, m = ext.conv1_fwd_relu(frames, w_rs, bias, 1.0)
        assert y.shape == (0, 32) and y.dtype == t.bfloat16
        assert m.shape == (0,) and m.dtype == t.int32
        for gw, gb in (ext.conv1_wrw(dy, frames, 1.0),
                       ext.conv1_wrw_masked(dy, mask, frames, 1.0)):
            assert gw.shape == (32, 4, 8, 8) and gw.dtype == t.float32
            assert gb.shape == (32,) and gb.dtype == t.float32
            assert not gw.any() and not gb.any()
        t.cuda.synchronize()
