// gfx950 per-step store of a vector env into the lane rings of the
// frame-deduplicated replay (DeviceVecFrameStackBuffer).
//
// E lanes (one per env), each a ring of S plane slots followed by a
// MIRROR of its first G = k + n slots: a row is R = S + G slots, and
// "write at slot i" means slot i and, when i < G, also slot S + i. A
// window that starts near the end of a row then runs on into the mirror
// and never wraps, which is what lets the gathers of framestack.hip
// read these rings as one flat ring [E*R, H, W] with base = position.
//
// One step of lane e, with i = head[e] mod S, bs = (i - k) mod S (the
// slot of the transition this step completes) and r = run[e] + 1:
//   plane i                = frame[e]
//   reward, terminal, left at bs = reward[e], terminal[e], 0
//   pos[e]                 = e*R + bs
//   leaf i                 -> 0        (its base plane is overwritten)
//   done[e] != 0:
//     j < min(n, r):  left at bs-j = j;  leaf bs-j -> fill
//     j < k:          plane i+1+j = first[e, j];  leaf i+1+j -> 0
//     head[e] += 1 + k;  run[e] = 0
//   else:
//     r >= n:         left at bs-(n-1) = n-1;  leaf bs-(n-1) -> fill
//     head[e] += 1;   run[e] = r
// (slots modulo S, non-negative). The leaves are not written here: the
// kernel returns them as a fixed-shape update list [E, k+1+n], zeroed
// leaves first, then filled ones, unused entries repeating (e*R + i, 0)
// so that duplicates carry equal weights.
//
// Work decomposition: one 256-thread workgroup per lane, grid capped at
// 2048 blocks and grid-strided over lanes. head, run and done are
// lane-uniform (readfirstlane); a barrier follows the reads and thread
// 0 writes head and run back. Pure byte movement:
// - vector path (H*W % 16 == 0, 16 B aligned ring and frame): dwordx4
//   loads and stores;
// - byte path (anything else, and a channels_last `first`): one pixel
//   per thread and pass. Only ended lanes read `first`, one lane in
//   the episode length per step, so its strided form is not vectorised.
// Every slot is reduced into [0, S) from head mod S by small offsets,
// so no value of head, run or done can address outside the lane's row.
// No LDS, no atomics, no scratch.
#include "common.h"

typedef unsigned char u8;
typedef uint32_t u32;

#define FV_BLOCK 256

struct fv_args {
  u8* __restrict__ planes;            // [E*R, HW]
  float* __restrict__ reward;         // [E*R]
  float* __restrict__ terminal;       // [E*R]
  int64_t* __restrict__ left;         // [E*R]
  int64_t* __restrict__ head;         // [E]
  int64_t* __restrict__ run;          // [E]
  const u8* __restrict__ frame;       // [E, HW]
  const u8* __restrict__ first;       // [E, k, HW] or [E, HW, k]
  const float* __restrict__ in_reward;    // [E]
  const float* __restrict__ in_terminal;  // [E]
  const float* __restrict__ done;     // [E]
  const float* __restrict__ fill;     // [1]
  int64_t* __restrict__ pos;          // [E]
  int64_t* __restrict__ leaf_idx;     // [E, k+1+n]
  float* __restrict__ leaf_w;         // [E, k+1+n]
  int64_t E, S, HW;
  int k, n;
  bool first_nhwc, first_vec;
};

__device__ __forceinline__ int64_t fv_uniform64(int64_t v) {
  const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
  const u32 hi =
      (u32)__builtin_amdgcn_readfirstlane((int)(u32)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// non-negative remainder
__device__ __forceinline__ int64_t fv_mod(int64_t a, int64_t S) {
  const int64_t r = a % S;
  return r < 0 ? r + S : r;
}

// the same for a in (-S, 2S): slots are offset by at most k + n < S
__device__ __forceinline__ int64_t fv_wrap(int64_t a, int64_t S) {
  return a < 0 ? a + S : (a >= S ? a - S : a);
}

// one plane into slot `slot` (< S) of a row, and into its mirror when
// slot < G; T is uint4 (C = HW/16) or u8 (C = HW, source stride in
// bytes). `slot` is block-uniform.
template <typename T>
__device__ __forceinline__ void fv_store_plane(T* __restrict__ row,
                                               const T* __restrict__ src,
                                               int64_t stride, int64_t slot,
                                               int64_t C, int64_t S, int G) {
  T* __restrict__ d = row + slot * C;
  if (slot < G) {
    T* __restrict__ m = row + (S + slot) * C;
    for (int64_t c = threadIdx.x; c < C; c += FV_BLOCK) {
      const T v = src[c * stride];
      d[c] = v;
      m[c] = v;
    }
  } else {
    for (int64_t c = threadIdx.x; c < C; c += FV_BLOCK)
      d[c] = src[c * stride];
  }
}

// one column entry at slot (< S) of the row that starts at col, and
// its mirror
template <typename T>
__device__ __forceinline__ void fv_store_col(T* __restrict__ column,
                                             int64_t col, int64_t slot,
                                             int64_t S, int G, T v) {
  column[col + slot] = v;
  if (slot < G) column[col + S + slot] = v;
}

template <bool VEC>
__global__ __launch_bounds__(FV_BLOCK) void framestack_vec_append_kernel(
    fv_args a) {
  const int k = a.k, n = a.n, G = k + n, L = k + 1 + n;
  const int64_t S = a.S, R = S + G, HW = a.HW, C16 = HW / 16;
  const int tid = threadIdx.x;
  for (int64_t e = blockIdx.x; e < a.E; e += gridDim.x) {
    const int64_t h = fv_uniform64(a.head[e]);
    const int64_t run = fv_uniform64(a.run[e]);
    const bool ended =
        __builtin_amdgcn_readfirstlane(a.done[e] != 0.0f ? 1 : 0) != 0;
    // all threads have read head[e] and run[e]; thread 0 may write them
    __syncthreads();
    const int64_t i = fv_mod(h, S);       // slot of this step's plane
    const int64_t bs = fv_wrap(i - k, S);  // slot of this step's transition
    const int64_t r = (int64_t)((uint64_t)run + 1u);
    const int64_t col = e * R;
    u8* row = a.planes + col * HW;

    // -- planes ------------------------------------------------------
    if (VEC) {
      fv_store_plane<uint4>((uint4*)row, (const uint4*)(a.frame + e * HW),
                            1, i, C16, S, G);
    } else {
      fv_store_plane<u8>(row, a.frame + e * HW, 1, i, HW, S, G);
    }
    if (ended) {
      for (int j = 0; j < k; ++j) {
        const int64_t slot = fv_wrap(i + 1 + j, S);
        if (VEC && a.first_vec) {
          fv_store_plane<uint4>(
              (uint4*)row, (const uint4*)(a.first + (e * k + j) * HW), 1,
              slot, C16, S, G);
        } else if (a.first_nhwc) {
          fv_store_plane<u8>(row, a.first + e * k * HW + j, k, slot, HW, S,
                             G);
        } else {
          fv_store_plane<u8>(row, a.first + (e * k + j) * HW, 1, slot, HW,
                             S, G);
        }
      }
    }

    // -- columns -----------------------------------------------------
    if (tid == 0) {
      fv_store_col<float>(a.reward, col, bs, S, G, a.in_reward[e]);
      fv_store_col<float>(a.terminal, col, bs, S, G, a.in_terminal[e]);
      a.pos[e] = col + bs;
      a.head[e] = (int64_t)((uint64_t)h + 1u + (ended ? (uint64_t)k : 0u));
      a.run[e] = ended ? 0 : r;
    }
    if (tid < n) {
      // thread j owns the transition j steps back
      const int j = tid;
      int64_t v = j == 0 ? 0 : -1;
      if (ended) {
        if (j < r) v = j;
      } else if (j == n - 1 && r >= n) {
        v = n - 1;
      }
      if (v >= 0)
        fv_store_col<int64_t>(a.left, col, fv_wrap(bs - j, S), S, G, v);
    }

    // -- leaf update list: entry 0 kills the leaf of the overwritten
    // plane, 1..k those of the next episode's first planes, k+1..k+n
    // fill the transitions that became sampleable
    if (tid < L) {
      int64_t slot = i;
      float w = 0.0f;
      if (tid >= 1 && tid <= k) {
        if (ended) slot = fv_wrap(i + tid, S);
      } else if (tid > k) {
        const int j = tid - k - 1;
        if (ended ? (j < r) : (j == 0 && r >= n)) {
          slot = fv_wrap(bs - (ended ? j : n - 1), S);
          w = a.fill[0];
        }
      }
      a.leaf_idx[e * L + tid] = col + slot;
      a.leaf_w[e * L + tid] = w;
    }
  }
}

// ---------------------------------------------------------------------
// host-side driver (called from bindings.cpp)
// ---------------------------------------------------------------------
void framestack_vec_append_launch(
    unsigned char* planes, float* reward, float* terminal, int64_t* left,
    int64_t* head, int64_t* run, const unsigned char* frame,
    const unsigned char* first, const float* in_reward,
    const float* in_terminal, const float* done, const float* fill,
    int64_t* pos, int64_t* leaf_idx, float* leaf_w, int64_t E, int64_t S,
    int64_t HW, int k, int n, bool first_nhwc, hipStream_t stream) {
  if (E == 0) return;
  fv_args a;
  a.planes = planes;
  a.reward = reward;
  a.terminal = terminal;
  a.left = left;
  a.head = head;
  a.run = run;
  a.frame = frame;
  a.first = first;
  a.in_reward = in_reward;
  a.in_terminal = in_terminal;
  a.done = done;
  a.fill = fill;
  a.pos = pos;
  a.leaf_idx = leaf_idx;
  a.leaf_w = leaf_w;
  a.E = E;
  a.S = S;
  a.HW = HW;
  a.k = k;
  a.n = n;
  a.first_nhwc = first_nhwc;
  // rows and planes are multiples of HW bytes: aligned when the ring is
  const bool vec = (HW % 16 == 0) &&
                   (((uintptr_t)planes | (uintptr_t)frame) & 15) == 0;
  a.first_vec = vec && !first_nhwc && ((uintptr_t)first & 15) == 0;
  const int grid = ma_grid(E * FV_BLOCK, FV_BLOCK);
  if (vec) {
    hipLaunchKernelGGL(framestack_vec_append_kernel<true>, dim3(grid),
                       dim3(FV_BLOCK), 0, stream, a);
  } else {
    hipLaunchKernelGGL(framestack_vec_append_kernel<false>, dim3(grid),
                       dim3(FV_BLOCK), 0, stream, a);
  }
}
