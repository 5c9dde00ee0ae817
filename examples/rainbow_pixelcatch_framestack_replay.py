"""RAINBOW on the built-in PixelCatch pixel env with FRAME-DEDUPLICATED
prioritized device replay and n-step returns folded WHEN SAMPLING.

`DeviceFrameStackBuffer(n_step=3)` stores the raw 1-step episode: every
84x84 frame once in an HBM ring (7 KB per transition instead of the
56 KB of two stacked `[4, 84, 84]` observations). Sampling is one
gfx950 kernel (`ops.framestack_gather_nstep`) that rebuilds `state` and
the n-step `next_state` stack and folds the n-step reward and terminal
of every sampled transition. RAINBOW sees that the buffer does the
n-step fold and skips its own per-transition host fold.

`replay_size` counts FRAMES here: an episode of L steps takes L + 4
ring slots. The buffer's `n_step` and `discount` must equal RAINBOW's
`reward_future_steps` and `discount`.

`--fused-loss` computes the whole C51 loss head (double-DQN action,
projection, cross entropy and their backward) with `ops.c51_loss`, one
gfx950 kernel each way, and bootstraps every sample with
`discount ** m` for the `m` steps its window really covers
(`exact_nstep_bootstrap`). `--logits` (implies `--fused-loss`) makes the
net return logits; the loss then takes `log_softmax` in fp32 inside the
kernel.

Runs on CPU too (the buffer and the loss fall back to torch ops), just
slower; on an MI355X pass --device cuda:0.

    python examples/rainbow_pixelcatch_framestack_replay.py [--device cuda:0]
        [--fused-loss] [--logits]
"""
import argparse
import os
import sys

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
)

import torch as t
import torch.nn as nn

from machin_amd.env.envs import PixelCatchEnv
from machin_amd.frame.algorithms import RAINBOW
from machin_amd.frame.buffers import DeviceFrameStackBuffer
from machin_amd.model.nets.nature_cnn import NatureCNN

N_STEP, DISCOUNT, ATOMS = 3, 0.99, 51


class DistQNet(nn.Module):
    """C51 head on the Nature CNN: [B, actions, atoms] probabilities,
    or logits with ``logits=True``."""

    def __init__(self, action_num=3, atom_num=ATOMS, logits=False):
        super().__init__()
        self.action_num, self.atom_num = action_num, atom_num
        self.logits = logits
        self.cnn = NatureCNN(4, feature_dim=256)
        self.head = nn.Linear(256, action_num * atom_num)

    def forward(self, state):
        a = self.head(self.cnn(state.float() / 255.0))
        a = a.view(-1, self.action_num, self.atom_num)
        return a if self.logits else t.softmax(a, dim=-1)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--device", default="cpu")
    parser.add_argument("--episodes", type=int, default=30)
    parser.add_argument("--replay-frames", type=int, default=20000)
    parser.add_argument("--fused-loss", action="store_true",
                        help="ops.c51_loss with discount ** m bootstrap")
    parser.add_argument("--logits", action="store_true",
                        help="the net returns logits (implies --fused-loss)")
    args = parser.parse_args()
    dev = t.device(args.device)
    fused = args.fused_loss or args.logits

    t.manual_seed(0)
    rainbow = RAINBOW(
        DistQNet(logits=args.logits).to(dev),
        DistQNet(logits=args.logits).to(dev), t.optim.Adam, -5.0, 5.0,
        batch_size=32,
        reward_future_steps=N_STEP,
        discount=DISCOUNT,
        # the interesting lines: raw frames are stored once, on the
        # device, and the n-step fold happens in the sampling kernel
        replay_buffer=DeviceFrameStackBuffer(
            args.replay_frames, args.device, frame_stack=4,
            prioritized=True, n_step=N_STEP, discount=DISCOUNT,
        ),
        epsilon_decay=0.999,
        fused_loss=fused,
        exact_nstep_bootstrap=fused,
        dist_from_logits=args.logits,
    )
    print("replay buffer:", type(rainbow.replay_buffer).__name__,
          "n_step", rainbow.replay_buffer.n_step,
          "fused loss", rainbow.fused_loss,
          "logits", rainbow.dist_from_logits)

    env = PixelCatchEnv(seed=0, balls=3)
    for ep in range(args.episodes):
        obs = env.reset()
        episode, total, done = [], 0.0, False
        while not done:
            # frames stay on the host: the whole episode goes up in
            # one copy when it is stored
            st = t.from_numpy(obs).unsqueeze(0)
            act = rainbow.act_discrete_with_noise({"state": st.to(dev)})
            obs2, r, done, _ = env.step(int(act.item()))
            total += r
            episode.append({
                "state": {"state": st},
                "action": {"action": act},
                "next_state": {"state": t.from_numpy(obs2).unsqueeze(0)},
                "reward": r,
                "terminal": done,
            })
            obs = obs2
        rainbow.store_episode(episode)
        losses = [rainbow.update() for _ in range(4)]
        print(f"ep {ep:3d} reward {total:+.0f} "
              f"loss {sum(losses) / len(losses):.4f} "
              f"eps {rainbow.epsilon:.3f} "
              f"replay {rainbow.replay_buffer.size()} transitions")


if __name__ == "__main__":
    main()
