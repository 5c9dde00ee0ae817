"""bench.py --dump-outputs: the writer of the last step's results."""
import os
import sys

import numpy as np
import pytest
import torch as t
import torch.nn as nn

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
)
from bench import dump_outputs  # noqa: E402


def test_dump_outputs_writes_loss_and_parameters(tmp_path):
    model = nn.Sequential(nn.Linear(3, 2), nn.Linear(2, 1)).to(t.bfloat16)
    loss = t.tensor(1.5, dtype=t.bfloat16)
    out = tmp_path / "nested" / "dump"
    dump_outputs(str(out), loss, model)

    names = sorted(p.name for p in out.iterdir())
    assert names == sorted(
        ["loss.npy"]
        + [f"param.{n}.npy" for n, _ in model.named_parameters()]
    )
    got = np.load(out / "loss.npy")
    assert got.dtype == np.float32 and got.shape == (1,)
    assert got[0] == 1.5
    for n, p in model.named_parameters():
        a = np.load(out / f"param.{n}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(p.shape)
        np.testing.assert_array_equal(a, p.detach().float().numpy())


@pytest.mark.gpu
def test_restore_state_makes_a_step_repeatable():
    """The dumped step runs from restored parameters and a fresh
    optimizer: it must then reproduce the very first step. Forward and
    loss have no float atomics, so the loss matches to fp32 rounding;
    the weight-gradient atomics reorder ~1e-7-relative terms of an
    update that is at most lr / eps * |g| / (|g| + 1) < 6e-3, so 1e-6
    absolute bounds the parameters with room to spare."""
    from bench import ImpalaLearnerBench

    b = ImpalaLearnerBench(
        device="cuda:0", unroll=8, env_batch=16, pool_size=1
    )
    snap = b.snapshot_state()
    first_loss = float(b.step())
    first = [p.detach().clone() for p in b.model.parameters()]
    b.step()
    b.step()

    b.restore_state(snap)
    for p, s in zip(b.model.parameters(), snap):
        assert t.equal(p, s)
    for st in b.optim.state.values():
        assert float(st["square_avg"].abs().max()) == 0.0

    again_loss = float(b.step())
    assert again_loss == pytest.approx(first_loss, rel=1e-5)
    for p, f in zip(b.model.parameters(), first):
        assert float((p.detach() - f).abs().max()) <= 1e-6
    moved = max(
        float((f - s).abs().max()) for f, s in zip(first, snap)
    )
    assert moved > 1e-4  # the step did move the parameters
