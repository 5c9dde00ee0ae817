"""IQN (implicit quantile networks) on 256 DEVICE-RESIDENT PixelCatch
envs.

This is `rainbow_pixelcatch_quantile.py` with sampled quantile
fractions: a `NatureCNN` torso and an `ImplicitQuantileHead` on noisy
layers, trained by `IQN`. Every forward draws `taus ~ U(0, 1)`; their
cosine embedding runs through `ops.iqn_embedding` (one gfx950 kernel
each way; a torch composition on the CPU) and the loss through
`ops.quantile_huber_loss(..., taus=taus)`.

    python examples/iqn_pixelcatch.py [--device cuda:0] [--envs 256]
        [--steps 300] [--quantiles 64] [--kappa 1.0]
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
from machin_amd.frame.algorithms import IQN
from machin_amd.frame.buffers import DeviceFrameStackBuffer
from machin_amd.model.nets import ImplicitQuantileHead, NatureCNN

N_STEP, DISCOUNT = 3, 0.99


class NoisyIQNNet(nn.Module):
    """Nature CNN torso, noisy IQN head: [B, actions, taus.shape[1]]."""

    def __init__(self, action_num=3, hidden=256):
        super().__init__()
        self.cnn = NatureCNN(4, feature_dim=256)
        self.head = ImplicitQuantileHead(256, action_num, hidden=hidden,
                                         noisy=True)

    def forward(self, state, taus):
        return self.head(self.cnn(state.float() / 255.0), taus)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--device", default="cpu")
    parser.add_argument("--envs", type=int, default=256)
    parser.add_argument("--steps", type=int, default=300,
                        help="vector steps (each is --envs env steps)")
    parser.add_argument("--balls", type=int, default=3)
    parser.add_argument("--quantiles", type=int, default=64)
    parser.add_argument("--kappa", type=float, default=1.0)
    parser.add_argument("--replay-frames", type=int, default=200000)
    args = parser.parse_args()
    dev = t.device(args.device)

    t.manual_seed(0)
    buffer = DeviceFrameStackBuffer(
        args.replay_frames, args.device, frame_stack=4, prioritized=True,
        n_step=N_STEP, discount=DISCOUNT,
    )
    iqn = IQN(
        NoisyIQNNet().to(dev), NoisyIQNNet().to(dev), t.optim.Adam,
        quantiles=args.quantiles, target_quantiles=args.quantiles,
        act_quantiles=32, huber_kappa=args.kappa,
        batch_size=32, reward_future_steps=N_STEP, discount=DISCOUNT,
        replay_buffer=buffer, exact_nstep_bootstrap=True, noisy_nets=True,
    )
    env = DevicePixelCatchVecEnv(
        args.envs, args.device, seed=0, balls=args.balls, record=True,
    )
    print(f"{env.size()} envs on {env.device}, episodes of {env.max_len} "
          f"steps, {args.quantiles} sampled fractions, kappa {args.kappa:g}")

    obs = env.reset()
    episodes, returns = 0, t.zeros((), device=dev)
    for step in range(args.steps):
        with t.no_grad():
            action = iqn.act_discrete_with_noise({"state": obs}).view(-1)
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
            loss = iqn.update()
            if step % 20 == 0 or step == args.steps - 1:
                print(f"step {step:4d} episodes {episodes:5d} "
                      f"mean return {float(returns) / max(episodes, 1):+.2f} "
                      f"loss {loss:.4f} replay {buffer.size()}")
    print(f"done: {episodes} episodes, replay {buffer.size()} transitions")
    env.close()


if __name__ == "__main__":
    main()
