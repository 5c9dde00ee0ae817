"""Full RAINBOW on 256 DEVICE-RESIDENT PixelCatch envs: noisy-network
exploration and a dueling C51 head on top of the device env, the
frame-deduplicated prioritized n-step replay and the fused loss.

This is `rainbow_pixelcatch_device_env.py` with the net swapped for
`NatureCNN + NoisyDuelingC51Head` (logits out) and the epsilon-greedy
code gone: `RAINBOW(noisy_nets=True)` draws new factorised noise for
the online net before every `act_discrete_with_noise` and for both nets
before every `update`, one `ops.factorised_noise_` launch per layer and
no host round trip; the noisy layers run through `ops.noisy_linear`
(fused gfx950 kernels at the update's batch of 32, the two-GEMM form at
the acting batch of 256).

Runs on CPU too (env, buffer, loss and layers fall back to torch ops),
just slower; on an MI355X pass --device cuda:0.

    python examples/rainbow_pixelcatch_noisy.py [--device cuda:0]
        [--envs 256] [--steps 300]
"""
import argparse
import os
import sys

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
)

import torch as t
import torch.nn as nn

from machin_amd.env.envs import DevicePixelCatchVecEnv
from machin_amd.frame.algorithms import RAINBOW
from machin_amd.frame.buffers import DeviceFrameStackBuffer
from machin_amd.model.nets import NatureCNN, NoisyDuelingC51Head

N_STEP, DISCOUNT, ATOMS = 3, 0.99, 51


class NoisyDuelingQNet(nn.Module):
    """Nature CNN torso, noisy dueling C51 head: [B, actions, atoms]
    logits."""

    def __init__(self, action_num=3, atom_num=ATOMS, hidden=256):
        super().__init__()
        self.cnn = NatureCNN(4, feature_dim=256)
        self.head = NoisyDuelingC51Head(256, action_num, atom_num,
                                        hidden=hidden)

    def forward(self, state):
        return self.head(self.cnn(state.float() / 255.0))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--device", default="cpu")
    parser.add_argument("--envs", type=int, default=256)
    parser.add_argument("--steps", type=int, default=300,
                        help="vector steps (each is --envs env steps)")
    parser.add_argument("--balls", type=int, default=3)
    parser.add_argument("--replay-frames", type=int, default=200000)
    parser.add_argument("--updates-per-step", type=int, default=1)
    args = parser.parse_args()
    dev = t.device(args.device)

    t.manual_seed(0)
    buffer = DeviceFrameStackBuffer(
        args.replay_frames, args.device, frame_stack=4, prioritized=True,
        n_step=N_STEP, discount=DISCOUNT,
    )
    rainbow = RAINBOW(
        NoisyDuelingQNet().to(dev), NoisyDuelingQNet().to(dev),
        t.optim.Adam, -5.0, 5.0,
        batch_size=32, reward_future_steps=N_STEP, discount=DISCOUNT,
        replay_buffer=buffer, fused_loss=True, dist_from_logits=True,
        noisy_nets=True,
    )
    env = DevicePixelCatchVecEnv(
        args.envs, args.device, seed=0, balls=args.balls, record=True,
    )
    print(f"{env.size()} envs on {env.device}, episodes of {env.max_len} "
          f"steps, log {env._log[0].numel() / 2 ** 20:.0f} MiB")

    obs = env.reset()
    episodes, returns = 0, t.zeros((), device=dev)
    for step in range(args.steps):
        # exploration is the online net's own noise: no epsilon
        with t.no_grad():
            action = rainbow.act_discrete_with_noise({"state": obs}).view(-1)
        obs, reward, done, _ = env.step(action)
        returns += reward.sum()
        for frames, cols in env.finished_episodes():
            buffer.store_frames(frames, {
                "action/action": cols["action"],
                "reward": cols["reward"],
                "terminal": cols["terminal"],
            })
            episodes += 1
        if buffer.size() >= 1000:
            losses = [rainbow.update()
                      for _ in range(args.updates_per_step)]
            if step % 20 == 0 or step == args.steps - 1:
                sigma = rainbow.qnet.head.advantage_out.weight_sigma
                print(f"step {step:4d} episodes {episodes:5d} "
                      f"mean return {float(returns) / max(episodes, 1):+.2f} "
                      f"loss {sum(losses) / len(losses):.4f} "
                      f"mean |sigma| {float(sigma.abs().mean()):.4f} "
                      f"replay {buffer.size()}")
    print(f"done: {episodes} episodes, replay {buffer.size()} transitions")
    env.close()


if __name__ == "__main__":
    main()
