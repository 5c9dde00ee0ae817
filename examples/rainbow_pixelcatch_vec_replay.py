"""RAINBOW on 256 DEVICE-RESIDENT PixelCatch envs with a PER-STEP store:
env, replay and learner live in HBM and the hop from the env to the
replay never waits for the device.

`examples/rainbow_pixelcatch_device_env.py` records whole episodes in
the env (`record=True`) and asks the host once per vector step which of
them ended. Here the env records nothing: every vector step goes
straight into `DeviceVecFrameStackBuffer(prioritized=True, n_step=3)`
with one `append_step` call — one gfx950 kernel
(`ops.framestack_vec_append`) that writes each env's newest plane into
its lane of the frame ring and keeps all bookkeeping (episode ends,
n-step windows, evictions) on the device. There is no
`finished_episodes()`, no per-episode python and no host read between
`env.step` and the replay; the loop condition uses the host counter
`steps_stored`. (`RAINBOW.update` still returns its loss as a float,
the one value a step of this loop reads back.)

Runs on CPU too (env, buffer and loss fall back to torch ops), just
slower; on an MI355X pass --device cuda:0.

    python examples/rainbow_pixelcatch_vec_replay.py [--device cuda:0]
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
from machin_amd.frame.buffers import DeviceVecFrameStackBuffer
from machin_amd.model.nets.nature_cnn import NatureCNN

N_STEP, DISCOUNT, ATOMS = 3, 0.99, 51


class DistQNet(nn.Module):
    """C51 head on the Nature CNN: [B, actions, atoms] probabilities."""

    def __init__(self, action_num=3, atom_num=ATOMS):
        super().__init__()
        self.action_num, self.atom_num = action_num, atom_num
        self.cnn = NatureCNN(4, feature_dim=256)
        self.head = nn.Linear(256, action_num * atom_num)

    def forward(self, state):
        a = self.head(self.cnn(state.float() / 255.0))
        return t.softmax(a.view(-1, self.action_num, self.atom_num), dim=-1)


def act_epsilon_greedy(rainbow, obs, epsilon):
    """One action per env, all on the device: greedy w.r.t. the online
    net, replaced by a uniform draw with probability epsilon PER ENV."""
    with t.no_grad():
        greedy = rainbow.act_discrete({"state": obs}).view(-1)
    explore = t.rand(greedy.shape, device=greedy.device) < epsilon
    random = t.randint(0, 3, greedy.shape, device=greedy.device)
    return t.where(explore, random, greedy)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--device", default="cpu")
    parser.add_argument("--envs", type=int, default=256)
    parser.add_argument("--steps", type=int, default=300,
                        help="vector steps (each is --envs env steps)")
    parser.add_argument("--balls", type=int, default=3)
    parser.add_argument("--lane-slots", type=int, default=512,
                        help="replay frames kept per env")
    parser.add_argument("--learn-after", type=int, default=8,
                        help="vector steps stored before learning starts")
    parser.add_argument("--updates-per-step", type=int, default=1)
    args = parser.parse_args()
    dev = t.device(args.device)

    t.manual_seed(0)
    buffer = DeviceVecFrameStackBuffer(
        args.envs, args.lane_slots, args.device, frame_stack=4,
        prioritized=True, n_step=N_STEP, discount=DISCOUNT,
    )
    rainbow = RAINBOW(
        DistQNet().to(dev), DistQNet().to(dev), t.optim.Adam, -5.0, 5.0,
        batch_size=32, reward_future_steps=N_STEP, discount=DISCOUNT,
        replay_buffer=buffer,
    )
    env = DevicePixelCatchVecEnv(
        args.envs, args.device, seed=0, balls=args.balls,
    )
    print(f"{env.size()} envs on {env.device}, episodes of {env.max_len} "
          f"steps, {args.lane_slots} replay frames per env")

    obs = env.reset()
    buffer.begin(obs)
    epsilon = 1.0
    returns = t.zeros((), device=dev)
    episodes = t.zeros((), device=dev)
    for step in range(args.steps):
        action = act_epsilon_greedy(rainbow, obs, epsilon)
        obs, reward, done, info = env.step(action)
        # the interesting line: one step of all envs, one call
        buffer.append_step(action, reward, done, info["frame"], obs)
        returns += reward.sum()
        episodes += done.sum()
        epsilon = max(0.05, epsilon * 0.995)
        if buffer.steps_stored >= args.learn_after:
            losses = [rainbow.update()
                      for _ in range(args.updates_per_step)]
            if step % 20 == 0 or step == args.steps - 1:
                # printing reads the counters back
                n = max(float(episodes), 1.0)
                print(f"step {step:4d} episodes {int(episodes):5d} "
                      f"mean return {float(returns) / n:+.2f} "
                      f"loss {sum(losses) / len(losses):.4f} "
                      f"eps {epsilon:.3f}")
    print(f"done: {int(episodes)} episodes, replay {buffer.size()} "
          f"transitions")
    env.close()


if __name__ == "__main__":
    main()
