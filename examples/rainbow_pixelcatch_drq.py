"""RAINBOW on device-resident PixelCatch envs with the random-shift
augmentation of DrQ / RAD / data-efficient Rainbow, at no extra pass
over the pixels.

This is `rainbow_pixelcatch_device_env.py` (env, replay and learner in
HBM) with one more argument: `DeviceFrameStackBuffer(augment_shift=4)`.
Every sampled batch is replicate-padded by 4 pixels and cropped back at
a random offset, drawn independently for `state` and `next_state`; the
shift is applied inside the frame-stack gather kernel that rebuilds the
stacks anyway, so sampling is still one launch and the ring keeps the
original frames. The offsets used come back with the batch as the
custom attribute `shift` (`[B, 4]` int32: dy_state, dx_state, dy_next,
dx_next), which RAINBOW ignores.

Runs on CPU too (env, buffer and loss fall back to torch ops), just
slower; on an MI355X pass --device cuda:0.

    python examples/rainbow_pixelcatch_drq.py [--device cuda:0]
        [--envs 256] [--steps 300] [--pad 4]
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
    """One action per env, all on the device (acting sees the frames as
    they are: only sampled batches are augmented)."""
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
    parser.add_argument("--replay-frames", type=int, default=200000)
    parser.add_argument("--updates-per-step", type=int, default=1)
    parser.add_argument("--pad", type=int, default=4,
                        help="augment_shift: shifts are uniform on "
                             "[-pad, pad] (0 turns the augmentation off)")
    parser.add_argument("--min-replay", type=int, default=1000,
                        help="transitions in the replay before updates")
    args = parser.parse_args()
    dev = t.device(args.device)

    t.manual_seed(0)
    buffer = DeviceFrameStackBuffer(
        args.replay_frames, args.device, frame_stack=4, prioritized=True,
        n_step=N_STEP, discount=DISCOUNT, augment_shift=args.pad,
    )
    rainbow = RAINBOW(
        DistQNet().to(dev), DistQNet().to(dev), t.optim.Adam, -5.0, 5.0,
        batch_size=32, reward_future_steps=N_STEP, discount=DISCOUNT,
        replay_buffer=buffer,
    )
    env = DevicePixelCatchVecEnv(
        args.envs, args.device, seed=0, balls=args.balls, record=True,
    )
    print(f"{env.size()} envs on {env.device}, random shift of "
          f"+/-{args.pad} pixels on every sampled batch")

    obs = env.reset()
    epsilon, episodes, returns = 1.0, 0, t.zeros((), device=dev)
    for step in range(args.steps):
        action = act_epsilon_greedy(rainbow, obs, epsilon)
        obs, reward, done, _ = env.step(action)
        returns += reward.sum()
        epsilon = max(0.05, epsilon * 0.995)
        for frames, cols in env.finished_episodes():
            buffer.store_frames(frames, {
                "action/action": cols["action"],
                "reward": cols["reward"],
                "terminal": cols["terminal"],
            })
            episodes += 1
        if buffer.size() >= args.min_replay:
            losses = [rainbow.update()
                      for _ in range(args.updates_per_step)]
            if step % 20 == 0 or step == args.steps - 1:
                print(f"step {step:4d} episodes {episodes:5d} "
                      f"mean return {float(returns) / max(episodes, 1):+.2f} "
                      f"loss {sum(losses) / len(losses):.4f} "
                      f"eps {epsilon:.3f} replay {buffer.size()}")
    if buffer.size() > 0:
        # what the augmentation did to one batch
        batch = buffer.sample_batch(8, sample_attrs=["state", "*"])[1]
        print("shift rows (dy_state, dx_state, dy_next, dx_next):",
              batch[1]["shift"].tolist() if args.pad else "off")
    print(f"done: {episodes} episodes, replay {buffer.size()} transitions")
    env.close()


if __name__ == "__main__":
    main()
