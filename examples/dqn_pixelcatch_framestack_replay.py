"""DQN on the built-in PixelCatch pixel env with FRAME-DEDUPLICATED
device replay: `DeviceFrameStackBuffer` stores every 84x84 frame once
in an HBM ring (7 KB per transition instead of the 56 KB of two
stacked `[4, 84, 84]` observations) and rebuilds the state/next_state
stacks at sampling time with one gfx950 kernel
(`ops.framestack_gather`).

`replay_size` counts FRAMES here: an episode of L steps takes L + 4
ring slots.

Runs on CPU too (the buffer falls back to torch ops), just slower; on
an MI355X pass --device cuda:0.

    python examples/dqn_pixelcatch_framestack_replay.py [--device cuda:0]
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
from machin_amd.frame.algorithms import DQN
from machin_amd.frame.buffers import DeviceFrameStackBuffer
from machin_amd.model.nets.nature_cnn import NatureCNN


class QNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.cnn = NatureCNN(4, feature_dim=256)
        self.head = nn.Linear(256, 3)

    def forward(self, state):
        return self.head(self.cnn(state.float() / 255.0))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--device", default="cpu")
    parser.add_argument("--episodes", type=int, default=30)
    parser.add_argument("--replay-frames", type=int, default=20000)
    args = parser.parse_args()
    dev = t.device(args.device)

    t.manual_seed(0)
    dqn = DQN(
        QNet().to(dev), QNet().to(dev), t.optim.Adam, nn.MSELoss(),
        batch_size=32,
        # the interesting line: frames are stored once, on the device
        replay_buffer=DeviceFrameStackBuffer(
            args.replay_frames, args.device, frame_stack=4
        ),
        epsilon_decay=0.999,
    )
    print("replay buffer:", type(dqn.replay_buffer).__name__)

    env = PixelCatchEnv(seed=0, balls=3)
    for ep in range(args.episodes):
        obs = env.reset()
        episode, total, done = [], 0.0, False
        while not done:
            # frames stay on the host: the whole episode goes up in
            # one copy when it is stored
            st = t.from_numpy(obs).unsqueeze(0)
            act = dqn.act_discrete_with_noise({"state": st.to(dev)})
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
        dqn.store_episode(episode)
        losses = [dqn.update() for _ in range(4)]
        print(f"ep {ep:3d} reward {total:+.0f} "
              f"loss {sum(losses) / len(losses):.4f} "
              f"eps {dqn.epsilon:.3f} "
              f"replay {dqn.replay_buffer.size()} transitions")


if __name__ == "__main__":
    main()
