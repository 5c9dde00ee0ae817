"""Shared helpers for the random-shift (DrQ) frame-stack tests: a second
formulation of the shift (replicate-pad on float, per-sample crop) that
never calls the code under test, the shift rows of the kernel tests,
and the buffer check run on the CPU and on the GPU."""
import torch as t
import torch.nn.functional as F

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -(2 ** 31)
BASES = [0, 3, 6, 7, 10, 10]


def ring(p, h, w, seed=0):
    gen = t.Generator().manual_seed(seed)
    return t.randint(0, 256, (p, h, w), dtype=t.uint8, generator=gen)


def pad_crop(stack, d, pad):
    """Replicate-pad ``stack`` (u8 ``[B, k, H, W]``) by ``pad`` and crop
    ``H x W`` at ``(pad + dy, pad + dx)`` per sample; ``d`` is ``[B, 2]``
    with ``|d| <= pad``."""
    B, _, H, W = stack.shape
    d = d.cpu().tolist()
    assert all(abs(v) <= pad for row in d for v in row)
    padded = F.pad(stack.cpu().float(), (pad, pad, pad, pad),
                   mode="replicate")
    rows = [
        padded[b, :, pad + dy : pad + dy + H, pad + dx : pad + dx + W]
        for b, (dy, dx) in enumerate(d)
    ]
    return t.stack(rows).to(t.uint8)


def random_shift(batch, pad, seed=0):
    gen = t.Generator().manual_seed(seed)
    return t.randint(-pad, pad + 1, (batch, 4), dtype=t.int32,
                     generator=gen)


def kernel_shift_rows():
    """``(base, shift)`` of the kernel cases: every byte alignment on
    both sides (dx 0, +/-1 .. +/-4), whole rows clamped (dx +/-8,
    +/-100), dy 0, +/-1, +/-3 and the int32 extremes; ``next_state``
    gets another pair than ``state`` in every row."""
    dxs = [0, 1, -1, 2, -2, 3, -3, 4, -4, 8, -8, 100, -100]
    pairs = [(dy, dx) for dy in (0, 1, -1, 3, -3) for dx in dxs]
    pairs += [(INT32_MAX, INT32_MIN), (INT32_MIN, INT32_MAX),
              (INT32_MAX, INT32_MAX), (INT32_MIN, INT32_MIN)]
    n = len(pairs)
    rows = [pairs[i] + pairs[(7 * i + 3) % n] for i in range(n)]
    shift = t.tensor(rows, dtype=t.int32)
    base = t.tensor([BASES[i % len(BASES)] for i in range(n)])
    return base, shift


def check_strides(got, want, channels_last):
    assert got.dtype == t.uint8 and got.shape == want.shape
    # strides of size-1 dims carry no layout information
    assert [s for s, n in zip(got.stride(), got.shape) if n > 1] == [
        s for s, n in zip(want.stride(), want.shape) if n > 1
    ]
    if channels_last:
        assert got.is_contiguous(memory_format=t.channels_last)
    else:
        assert got.is_contiguous()


# -- buffer ---------------------------------------------------------------
LENGTHS = [5, 7, 1, 9]  # 22 transitions, 38 planes: nothing is evicted


def check_buffer(device, n_step, prioritized, layout, pad=2, batch=64):
    """Every sampled row is the shift, by the returned ``shift`` row, of
    the ORIGINAL stacks of its transition; the ring is left as it was."""
    from machin_amd.frame.buffers import DeviceFrameStackBuffer

    kwargs = dict(prioritized=prioritized, frame_layout=layout,
                  augment_shift=pad)
    if n_step == 1:
        from util_framestack import ATTRS, Episodes

        eps = Episodes()
        buf = DeviceFrameStackBuffer(40, device, **kwargs)
        for length in LENGTHS:
            buf.store_episode(eps.make(length)[0])
        want_state = t.stack(eps.state)
        want_next = t.stack(eps.next_state)
        attrs = ATTRS + ["*"]
    else:
        from util_framestack_nstep import ATTRS as attrs
        from util_framestack_nstep import host_fold, make_episodes

        episodes = make_episodes(LENGTHS)
        rows = host_fold(episodes, n_step, 0.5)
        buf = DeviceFrameStackBuffer(40, device, n_step=n_step,
                                     discount=0.5, **kwargs)
        for episode in episodes:
            buf.store_episode(episode)
        want_state, want_next = rows["state/state"], rows["next_state/state"]
    planes_before = buf._planes.clone()
    t.manual_seed(3)
    out = buf.sample_batch(batch, sample_attrs=attrs)
    assert out[0] == batch
    state, _, reward, next_state, _, others = out[1]
    shift = others["shift"]
    assert shift.dtype == t.int32 and shift.shape == (batch, 4)
    assert shift.device == buf._planes.device
    assert 0 < int(shift.abs().max()) <= pad
    if n_step == 1:
        assert set(others) == {"shift"}
        ids = reward.view(-1).cpu().long()
    else:
        assert set(others) == {"tid", "n_step", "shift"}
        ids = others["tid"].view(-1).cpu().long()
        assert t.equal(reward.view(-1).cpu(), rows["reward"][ids])
        assert t.equal(others["n_step"].view(-1).cpu(), rows["m"][ids])
    for got, want, cols in ((state["state"], want_state, shift[:, 0:2]),
                            (next_state["state"], want_next, shift[:, 2:4])):
        assert got.device == buf._planes.device and got.dtype == t.uint8
        if layout == "nhwc":
            assert got.is_contiguous(memory_format=t.channels_last)
        else:
            assert got.is_contiguous()
        assert t.equal(got.cpu(), pad_crop(want[ids], cols, pad))
    assert t.equal(buf._planes, planes_before)
    return buf, shift
