"""Device-resident sum-tree (GPU twin of frame.buffers.WeightTree).

Same heap layout as the CPU tree: one float32 tensor of length
2*capacity, root at index 1, leaves at [capacity, 2*capacity). All
operations are HIP kernels (machin_amd/ops/hip/sumtree.hip); nothing
synchronizes with the host except explicit scalar reads.

Reference CPU baselines this must beat (BASELINE.md / reference
machin/frame/buffers/prioritized_buffer.py:32-40): build 10M leaves
90 ms, 10M lookups 230 ms, 1M batched update 20 ms.
"""
import math
from typing import Union

import torch as t

from . import _require_ext


class DeviceSumTree:
    """Sum-tree over ``size`` leaves stored on a ROCm device."""

    def __init__(self, size: int, device: Union[str, t.device] = "cuda:0"):
        if size <= 0:
            raise ValueError("Tree size must be positive.")
        self.size = int(size)
        self.depth = max(1, int(math.ceil(math.log2(max(self.size, 2)))))
        self.capacity = 1 << self.depth
        self.device = t.device(device)
        self.weights = t.zeros(
            2 * self.capacity, dtype=t.float32, device=self.device
        )
        # CUDA tensors REQUIRE the gfx950 extension (no silent eager
        # fallback on a GPU box); a CPU-device tree runs the torch
        # fallback below so the device data path is testable in
        # CPU-only CI (gloo multi-process tests).
        self._ext = _require_ext() if self.device.type == "cuda" else None

    # -- accessors -----------------------------------------------------
    def get_weight_sum(self) -> float:
        return float(self.weights[1].item())

    def get_weight_sum_tensor(self) -> t.Tensor:
        """Root weight as a 0-dim device tensor (no host sync)."""
        return self.weights[1]

    def get_leaf_all_weights(self) -> t.Tensor:
        return self.weights[self.capacity : self.capacity + self.size]

    def get_leaf_weight(self, index: t.Tensor) -> t.Tensor:
        index = index.to(device=self.device, dtype=t.long)
        return self.weights[self.capacity + index]

    def get_leaf_max(self) -> float:
        if self.size == 0:
            return 0.0
        return float(self.get_leaf_all_weights().max().item())

    # -- updates -------------------------------------------------------
    def update_leaf_batch(self, weights: t.Tensor, indexes: t.Tensor):
        weights = weights.to(device=self.device, dtype=t.float32).contiguous()
        indexes = indexes.to(device=self.device, dtype=t.long).contiguous()
        if self._ext is None:
            self.weights[self.capacity + indexes] = weights
            self._rebuild_cpu()
            return
        self._ext.sumtree_update(
            self.weights, indexes, weights, self.capacity, self.depth
        )

    def _rebuild_cpu(self):
        """Full bottom-up rebuild (CPU fallback path)."""
        base, size = self.capacity, self.capacity
        while size > 1:
            parents = self.weights[base : base + size].view(-1, 2).sum(1)
            self.weights[base // 2 : base // 2 + size // 2] = parents
            base //= 2
            size //= 2

    def update_all_leaves(self, weights: t.Tensor):
        if weights.numel() != self.size:
            raise ValueError(f"Expected {self.size} weights.")
        leaves = self.weights[self.capacity : self.capacity + self.size]
        leaves.copy_(weights.to(device=self.device, dtype=t.float32))
        if self._ext is None:
            self._rebuild_cpu()
            return
        self._ext.sumtree_build(self.weights, self.capacity)

    # -- queries -------------------------------------------------------
    def find_leaf_index(self, prefix_weights: t.Tensor) -> t.Tensor:
        """Map prefix weights in the closed range [0, sum] to leaf
        indexes.

        The walk, the same on the device and in the CPU path: at each
        node with children ``(lw, rw)`` and running prefix ``w``, go
        right iff ``rw > 0 and (w > lw or lw <= 0)`` and then subtract
        ``lw``; a tie ``w == lw`` stays left. With fp32 prefix sums
        ``c`` leaf ``i`` therefore answers ``c[i-1] < u <= c[i]``, and
        a subtree of zero weight is never entered: as long as the tree
        holds any weight, no query (``0`` and ``sum`` included) returns
        a zero-weight or padding leaf.
        """
        u = prefix_weights.to(device=self.device, dtype=t.float32).contiguous()
        if self._ext is None:
            u = u.clone()
            idx = t.ones_like(u, dtype=t.long)
            for _ in range(self.depth):
                left = self.weights[2 * idx]
                right = (self.weights[2 * idx + 1] > 0) & (
                    (u > left) | ~(left > 0)
                )
                u = u - left * right
                idx = 2 * idx + right.long()
            return (idx - self.capacity).clamp_(0, self.size - 1)
        return self._ext.sumtree_sample(
            self.weights, u, self.capacity, self.depth, self.size
        )

    def sample(self, n: int, stratified: bool = True) -> t.Tensor:
        """Draw ``n`` leaves proportional to weight, fully on device."""
        total = self.get_weight_sum_tensor()
        if stratified:
            u = (
                t.rand(n, device=self.device, dtype=t.float32)
                + t.arange(n, device=self.device, dtype=t.float32)
            ) * (total / n)
        else:
            u = t.rand(n, device=self.device, dtype=t.float32) * total
        return self.find_leaf_index(u)
