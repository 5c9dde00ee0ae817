// gfx950 frame-stack gather for frame-deduplicated replay.
//
// The replay stores every frame ONCE in a ring of u8 planes [P, H, W].
// A sampled transition b owns the k+1 consecutive ring slots
// (base[b] + j) mod P, j = 0..k: planes 0..k-1 are its state stack,
// planes 1..k its next_state stack. This kernel rebuilds both stacks
// in one pass: each plane is loaded once per sample and stored to its
// one or two destinations (k+1 plane reads + 2k plane writes per
// sample; the torch composition index_select -> two slices ->
// two layout copies moves about twice that in 4-5 launches).
//
// Pure byte movement, memory-bound (guide §6 G13: 16 B/lane):
// - vector path (H*W % 16 == 0, 16 B aligned ring): one work item =
//   16 pixels of one sample, k+1 dwordx4 loads;
//     NCHW: each loaded plane chunk goes out as dwordx4 stores;
//     NHWC, k == 4: the 4x16 bytes are transposed in registers with
//     v_perm_b32 and leave as four dwordx4 stores per stack.
// - scalar path (any other H*W, other k in NHWC): one work item = one
//   pixel of one sample.
// No LDS, no atomics. `base` is reduced into [0, P) in the kernel
// (non-negative modulo), so no int64 value can address outside the
// ring and the host never has to look at the values.
//
// The second half of the file is the n-step variant of the same
// gather (framestack_gather_nstep_launch).
#include "common.h"

typedef unsigned char u8;
typedef uint32_t u32;

#define FS_MAX_K 8

// ring slot of window plane j: s in [0, P), j <= k < P  ->  s + j < 2P
__device__ __forceinline__ int64_t fs_slot(int64_t s, int j, int64_t P) {
  int64_t r = s + j;
  return r >= P ? r - P : r;
}

__device__ __forceinline__ int64_t fs_base(const int64_t* __restrict__ base,
                                           int64_t b, int64_t P) {
  int64_t s = base[b] % P;
  return s < 0 ? s + P : s;
}

// ---------------------------------------------------------------------
// NCHW vector path. C = H*W/16 chunks per plane; out index of chunk c
// of channel j of sample b is (b*K + j)*C + c.
// ---------------------------------------------------------------------
template <int K>
__global__ void framestack_nchw_vec_kernel(const uint4* __restrict__ planes,
                                           const int64_t* __restrict__ base,
                                           uint4* __restrict__ state,
                                           uint4* __restrict__ next,
                                           int64_t B, int64_t P, int64_t C) {
  const int64_t total = B * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / C, c = i - b * C;
    const int64_t s = fs_base(base, b, P);
    uint4 v[K + 1];
#pragma unroll
    for (int j = 0; j <= K; ++j) v[j] = planes[fs_slot(s, j, P) * C + c];
    const int64_t o = b * K * C + c;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      state[o + j * C] = v[j];
      next[o + j * C] = v[j + 1];
    }
  }
}

// ---------------------------------------------------------------------
// NHWC k == 4 vector path: 4x4 byte transposes with v_perm_b32.
// __builtin_amdgcn_perm(hi, lo, sel): result byte n = byte sel[n] of
// the 8-byte value {hi, lo} (selectors 0-3 -> lo, 4-7 -> hi).
// ---------------------------------------------------------------------
// words a,b,c,d hold 4 pixels of channels 0..3; o[q] = pixel q's
// 4 channel bytes (a_q, b_q, c_q, d_q).
__device__ __forceinline__ void fs_transpose4(u32 a, u32 b, u32 c, u32 d,
                                              u32 o[4]) {
  u32 ab_lo = __builtin_amdgcn_perm(b, a, 0x05010400u);  // a0 b0 a1 b1
  u32 ab_hi = __builtin_amdgcn_perm(b, a, 0x07030602u);  // a2 b2 a3 b3
  u32 cd_lo = __builtin_amdgcn_perm(d, c, 0x05010400u);  // c0 d0 c1 d1
  u32 cd_hi = __builtin_amdgcn_perm(d, c, 0x07030602u);  // c2 d2 c3 d3
  o[0] = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u);
  o[1] = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u);
  o[2] = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u);
  o[3] = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u);
}

__device__ __forceinline__ u32 fs_word(const uint4& v, int g) {
  return g == 0 ? v.x : g == 1 ? v.y : g == 2 ? v.z : v.w;
}

// 16 pixels x 4 channels -> 64 interleaved bytes = 4 dwordx4 stores
__device__ __forceinline__ void fs_store_nhwc4(uint4* __restrict__ dst,
                                               const uint4& p0,
                                               const uint4& p1,
                                               const uint4& p2,
                                               const uint4& p3) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    u32 o[4];
    fs_transpose4(fs_word(p0, g), fs_word(p1, g), fs_word(p2, g),
                  fs_word(p3, g), o);
    dst[g] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

__global__ void framestack_nhwc4_vec_kernel(const uint4* __restrict__ planes,
                                            const int64_t* __restrict__ base,
                                            uint4* __restrict__ state,
                                            uint4* __restrict__ next,
                                            int64_t B, int64_t P,
                                            int64_t C) {
  const int64_t total = B * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / C, c = i - b * C;
    const int64_t s = fs_base(base, b, P);
    uint4 v[5];
#pragma unroll
    for (int j = 0; j <= 4; ++j) v[j] = planes[fs_slot(s, j, P) * C + c];
    // sample b holds C*4 uint4 per stack; item i owns uint4 [4i, 4i+4)
    fs_store_nhwc4(state + 4 * i, v[0], v[1], v[2], v[3]);
    fs_store_nhwc4(next + 4 * i, v[1], v[2], v[3], v[4]);
  }
}

// ---------------------------------------------------------------------
// scalar path: one work item = one pixel of one sample, any H*W, any
// k <= FS_MAX_K, both layouts.
// ---------------------------------------------------------------------
__global__ void framestack_scalar_kernel(const u8* __restrict__ planes,
                                         const int64_t* __restrict__ base,
                                         u8* __restrict__ state,
                                         u8* __restrict__ next, int64_t B,
                                         int64_t P, int64_t HW, int k,
                                         bool nhwc) {
  const int64_t total = B * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / HW, px = i - b * HW;
    const int64_t s = fs_base(base, b, P);
    // element (b, j, px): NCHW (b*k + j)*HW + px, NHWC (b*HW + px)*k + j
    const int64_t o = nhwc ? i * k : b * k * HW + px;
    const int64_t step = nhwc ? 1 : HW;
    for (int j = 0; j <= k; ++j) {
      u8 v = planes[fs_slot(s, j, P) * HW + px];
      if (j < k) state[o + j * step] = v;
      if (j >= 1) next[o + (j - 1) * step] = v;
    }
  }
}

// ---------------------------------------------------------------------
// host-side driver (called from bindings.cpp)
// ---------------------------------------------------------------------
template <int K>
static void fs_launch_nchw_vec(const u8* planes, const int64_t* base,
                               u8* state, u8* next, int64_t B, int64_t P,
                               int64_t C, hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(framestack_nchw_vec_kernel<K>,
                     dim3(ma_grid(B * C, block)), dim3(block), 0, stream,
                     (const uint4*)planes, base, (uint4*)state,
                     (uint4*)next, B, P, C);
}

void framestack_gather_launch(const unsigned char* planes,
                              const int64_t* base, unsigned char* state,
                              unsigned char* next, int64_t B, int64_t P,
                              int64_t HW, int k, bool nhwc,
                              hipStream_t stream) {
  if (B == 0 || HW == 0) return;
  const int block = 256;
  const bool aligned =
      (((uintptr_t)planes | (uintptr_t)state | (uintptr_t)next) & 15) == 0;
  const bool vec = (HW % 16 == 0) && aligned;
  const int64_t C = HW / 16;
  if (vec && !nhwc) {
    switch (k) {
      case 1: fs_launch_nchw_vec<1>(planes, base, state, next, B, P, C, stream); return;
      case 2: fs_launch_nchw_vec<2>(planes, base, state, next, B, P, C, stream); return;
      case 3: fs_launch_nchw_vec<3>(planes, base, state, next, B, P, C, stream); return;
      case 4: fs_launch_nchw_vec<4>(planes, base, state, next, B, P, C, stream); return;
      case 5: fs_launch_nchw_vec<5>(planes, base, state, next, B, P, C, stream); return;
      case 6: fs_launch_nchw_vec<6>(planes, base, state, next, B, P, C, stream); return;
      case 7: fs_launch_nchw_vec<7>(planes, base, state, next, B, P, C, stream); return;
      case 8: fs_launch_nchw_vec<8>(planes, base, state, next, B, P, C, stream); return;
      default: break;
    }
  }
  if (vec && nhwc && k == 4) {
    hipLaunchKernelGGL(framestack_nhwc4_vec_kernel,
                       dim3(ma_grid(B * C, block)), dim3(block), 0, stream,
                       (const uint4*)planes, base, (uint4*)state,
                       (uint4*)next, B, P, C);
    return;
  }
  hipLaunchKernelGGL(framestack_scalar_kernel,
                     dim3(ma_grid(B * HW, block)), dim3(block), 0, stream,
                     planes, base, state, next, B, P, HW, k, nhwc);
}

// =====================================================================
// n-step gather: n-step returns computed WHEN SAMPLING, from raw
// 1-step episodes. The kernel gets the whole transition-ring columns
// base/left/reward/terminal [T] and the sampled ring positions pos [B]
// and indexes the columns itself. For sample b:
//   p = pos[b] mod T,  s = base[p] mod P,
//   m = clamp(left[p], 0, n-1) + 1        (transitions in the window)
//   state[b, j]      = planes[(s + j) mod P]
//   next_state[b, j] = planes[(s + m + j) mod P]          j < k
//   reward_n[b]   = sum_{j<m} gamma^j reward[q_j] prod_{i<j} (1 - terminal[q_i])
//   terminal_n[b] = max_{j<m} terminal[q_j],   q_j = (p + j) mod T
//   steps[b]      = m
// Every index is reduced or clamped in the kernel, so no value of pos,
// base or left can address outside either ring (P >= k + n is checked
// by the binding: s + m + j < 2P for fs_slot).
//
// Same work decomposition as above (one item = 16 pixels, or one
// pixel, of one sample); every item reads base[p] and left[p] (two
// cached 8-byte loads), and the item that owns chunk 0 of a sample
// also walks its <= n reward/terminal entries and writes the three
// per-sample scalars. One launch, no LDS, no atomics.
// =====================================================================
struct fs_nstep_args {
  const int64_t* __restrict__ base;     // [T]
  const int64_t* __restrict__ left;     // [T]
  const float* __restrict__ reward;     // [T]
  const float* __restrict__ terminal;   // [T]
  const int64_t* __restrict__ pos;      // [B]
  float* __restrict__ reward_n;         // [B]
  float* __restrict__ terminal_n;       // [B]
  int64_t* __restrict__ steps;          // [B]
  int64_t B, P, T;
  int n;
  float gamma;
};

// p, s and m of sample b
__device__ __forceinline__ void fs_nstep_window(const fs_nstep_args& a,
                                                int64_t b, int64_t& p,
                                                int64_t& s, int& m) {
  p = a.pos[b] % a.T;
  if (p < 0) p += a.T;
  s = fs_base(a.base, p, a.P);
  int64_t l = a.left[p];
  l = l < 0 ? 0 : (l > a.n - 1 ? a.n - 1 : l);
  m = (int)l + 1;
}

// the three per-sample scalars (called by one item per sample)
__device__ __forceinline__ void fs_nstep_scalars(const fs_nstep_args& a,
                                                 int64_t b, int64_t p,
                                                 int m) {
  float acc = 0.0f, disc = 1.0f, tmax = 0.0f;
  int64_t q = p;
  for (int j = 0; j < m; ++j) {
    const float r = a.reward[q], d = a.terminal[q];
    acc += disc * r;
    tmax = j == 0 ? d : fmaxf(tmax, d);
    disc *= a.gamma * (1.0f - d);
    if (++q == a.T) q = 0;
  }
  a.reward_n[b] = acc;
  a.terminal_n[b] = tmax;
  a.steps[b] = m;
}

// Vector paths: 2k dwordx4 loads per item, k for each stack. When
// m < k the stacks share k - m planes; the second load of a shared
// chunk comes from the same lane and is served by the cache, so HBM
// traffic is k + min(m, k) plane reads. Keeping the shared chunks in
// registers instead (k + m loads, one compile-time case per m < k)
// was measured and is not faster: docs/PERFORMANCE.md.
template <int K>
__global__ void framestack_nstep_nchw_vec_kernel(
    const uint4* __restrict__ planes, uint4* __restrict__ state,
    uint4* __restrict__ next, fs_nstep_args a, int64_t C) {
  const int64_t total = a.B * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / C, c = i - b * C;
    int64_t p, s;
    int m;
    fs_nstep_window(a, b, p, s, m);
    uint4 v[K], w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      v[j] = planes[fs_slot(s, j, a.P) * C + c];
      w[j] = planes[fs_slot(s, m + j, a.P) * C + c];
    }
    const int64_t o = b * K * C + c;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      state[o + j * C] = v[j];
      next[o + j * C] = w[j];
    }
    if (c == 0) fs_nstep_scalars(a, b, p, m);
  }
}

// NHWC k == 4 vector path
__global__ void framestack_nstep_nhwc4_vec_kernel(
    const uint4* __restrict__ planes, uint4* __restrict__ state,
    uint4* __restrict__ next, fs_nstep_args a, int64_t C) {
  const int64_t total = a.B * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / C, c = i - b * C;
    int64_t p, s;
    int m;
    fs_nstep_window(a, b, p, s, m);
    uint4 v[4], w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = planes[fs_slot(s, j, a.P) * C + c];
      w[j] = planes[fs_slot(s, m + j, a.P) * C + c];
    }
    fs_store_nhwc4(state + 4 * i, v[0], v[1], v[2], v[3]);
    fs_store_nhwc4(next + 4 * i, w[0], w[1], w[2], w[3]);
    if (c == 0) fs_nstep_scalars(a, b, p, m);
  }
}

// scalar path: one work item = one pixel of one sample
__global__ void framestack_nstep_scalar_kernel(
    const u8* __restrict__ planes, u8* __restrict__ state,
    u8* __restrict__ next, fs_nstep_args a, int64_t HW, int k, bool nhwc) {
  const int64_t total = a.B * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / HW, px = i - b * HW;
    int64_t p, s;
    int m;
    fs_nstep_window(a, b, p, s, m);
    const int64_t o = nhwc ? i * k : b * k * HW + px;
    const int64_t step = nhwc ? 1 : HW;
    for (int j = 0; j < k; ++j) {
      state[o + j * step] = planes[fs_slot(s, j, a.P) * HW + px];
      next[o + j * step] = planes[fs_slot(s, m + j, a.P) * HW + px];
    }
    if (px == 0) fs_nstep_scalars(a, b, p, m);
  }
}

template <int K>
static void fs_launch_nstep_nchw_vec(const u8* planes, u8* state, u8* next,
                                     const fs_nstep_args& a, int64_t C,
                                     hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(framestack_nstep_nchw_vec_kernel<K>,
                     dim3(ma_grid(a.B * C, block)), dim3(block), 0, stream,
                     (const uint4*)planes, (uint4*)state, (uint4*)next, a,
                     C);
}

void framestack_gather_nstep_launch(
    const unsigned char* planes, const int64_t* base, const int64_t* left,
    const float* reward, const float* terminal, const int64_t* pos,
    unsigned char* state, unsigned char* next, float* reward_n,
    float* terminal_n, int64_t* steps, int64_t B, int64_t P, int64_t T,
    int64_t HW, int k, int n, float gamma, bool nhwc, hipStream_t stream) {
  if (B == 0) return;
  const fs_nstep_args a = {base,     left,       reward, terminal, pos,
                           reward_n, terminal_n, steps,  B,        P,
                           T,        n,          gamma};
  const int block = 256;
  const bool aligned =
      (((uintptr_t)planes | (uintptr_t)state | (uintptr_t)next) & 15) == 0;
  const bool vec = (HW % 16 == 0) && aligned;
  const int64_t C = HW / 16;
  if (vec && !nhwc) {
    switch (k) {
      case 1: fs_launch_nstep_nchw_vec<1>(planes, state, next, a, C, stream); return;
      case 2: fs_launch_nstep_nchw_vec<2>(planes, state, next, a, C, stream); return;
      case 3: fs_launch_nstep_nchw_vec<3>(planes, state, next, a, C, stream); return;
      case 4: fs_launch_nstep_nchw_vec<4>(planes, state, next, a, C, stream); return;
      case 5: fs_launch_nstep_nchw_vec<5>(planes, state, next, a, C, stream); return;
      case 6: fs_launch_nstep_nchw_vec<6>(planes, state, next, a, C, stream); return;
      case 7: fs_launch_nstep_nchw_vec<7>(planes, state, next, a, C, stream); return;
      case 8: fs_launch_nstep_nchw_vec<8>(planes, state, next, a, C, stream); return;
      default: break;
    }
  }
  if (vec && nhwc && k == 4) {
    hipLaunchKernelGGL(framestack_nstep_nhwc4_vec_kernel,
                       dim3(ma_grid(B * C, block)), dim3(block), 0, stream,
                       (const uint4*)planes, (uint4*)state, (uint4*)next, a,
                       C);
    return;
  }
  hipLaunchKernelGGL(framestack_nstep_scalar_kernel,
                     dim3(ma_grid(B * HW, block)), dim3(block), 0, stream,
                     planes, state, next, a, HW, k, nhwc);
}

// =====================================================================
// Random-shift augmentation (DrQ / RAD) fused into both gathers.
// shift is int32 [B, 4] = (dy_state, dx_state, dy_next, dx_next); with
// S the stack the un-shifted gather returns,
//   out[b, j, y, x] = S[b, j, clamp(y + dy, 0, H-1), clamp(x + dx, 0, W-1)]
// which for |d| <= pad is "replicate-pad by pad, crop H x W at
// (pad + dy, pad + dx)". One (dy, dx) per stack, all k planes. dy is
// clamped into [-(H-1), H-1] and dx into [-(W-1), W-1] before the add
// (same result), so no int32 value overflows or leaves a plane. Window
// indices are reduced exactly as in the kernels above; the 1-step
// gather is the n-step one with m = 1 and no scalars (NSTEP == false:
// only a.base, a.B and a.P are set).
//
// - vector path (W % 4 == 0, 4 B aligned ring): one work item = one
//   output dword = 4 pixels of one row of one sample, all planes of
//   both stacks. The 4 source pixels clamp(x0 + q, 0, W-1), x0 = 4*xd +
//   dx, always lie in the dword pair (a, min(a + 1, W/4 - 1)) with
//   a = clamp(floor(x0 / 4), 0, W/4 - 1): an interior dword straddles
//   two dwords, and a dword cut by a row end takes all its bytes from
//   the row's first or last dword. So every output dword is two aligned
//   dword loads and one v_perm_b32 whose byte selectors
//   clamp(x0 + q, 0, W-1) - 4a (in [0, 7]) are computed once per stack:
//   no branch, no byte loads.
//     NCHW: one dword store per plane, consecutive lanes on
//     consecutive dwords;
//     NHWC, k == 4: 4 pixels x 4 channels = one dwordx4 store per
//     stack through fs_transpose4.
//   state and next_state have different shifts, so a plane they share
//   is loaded once per stack; the second load comes from cache.
// - scalar path (any other W, NHWC with k != 4): one pixel per item.
// No LDS, no atomics, no scratch.
// =====================================================================
__device__ __forceinline__ int fs_clampi(int v, int lo, int hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// where one stack's output dword (row y, dword xd) comes from: dword
// offsets of the pair inside a plane and the v_perm_b32 selector
struct fs_shift_src {
  int lo, hi;
  u32 sel;
};

__device__ __forceinline__ fs_shift_src fs_shift_dword(
    const int* __restrict__ sh, int y, int xd, int H, int W) {
  const int Wd = W >> 2;
  const int dy = fs_clampi(sh[0], -(H - 1), H - 1);
  const int dx = fs_clampi(sh[1], -(W - 1), W - 1);
  const int ys = fs_clampi(y + dy, 0, H - 1);
  const int x0 = 4 * xd + dx;  // |x0| < 2W
  const int a = fs_clampi(x0 >> 2, 0, Wd - 1);
  fs_shift_src r;
  r.lo = ys * Wd + a;
  r.hi = ys * Wd + (a + 1 < Wd ? a + 1 : Wd - 1);
  r.sel = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    r.sel |= (u32)(fs_clampi(x0 + q, 0, W - 1) - 4 * a) << (8 * q);
  return r;
}

__device__ __forceinline__ u32 fs_shift_load(const u32* __restrict__ plane,
                                             const fs_shift_src& r) {
  return __builtin_amdgcn_perm(plane[r.hi], plane[r.lo], r.sel);
}

// window of sample b: 1-step (base is indexed by b) or n-step
template <bool NSTEP>
__device__ __forceinline__ void fs_shift_window(const fs_nstep_args& a,
                                                int64_t b, int64_t& p,
                                                int64_t& s, int& m) {
  if (NSTEP) {
    fs_nstep_window(a, b, p, s, m);
  } else {
    p = b;
    s = fs_base(a.base, b, a.P);
    m = 1;
  }
}

// NCHW vector path. C = H*W/4 dwords per plane; out dword c of channel
// j of sample b is (b*K + j)*C + c.
template <int K, bool NSTEP>
__global__ void framestack_shift_nchw_vec_kernel(
    const u32* __restrict__ planes, const int* __restrict__ shift,
    u32* __restrict__ state, u32* __restrict__ next, fs_nstep_args a,
    int H, int W) {
  const int Wd = W >> 2;
  const int64_t C = (int64_t)H * Wd;
  const int64_t total = a.B * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / C;
    const int c = (int)(i - b * C);
    const int y = c / Wd, xd = c - y * Wd;
    int64_t p, s;
    int m;
    fs_shift_window<NSTEP>(a, b, p, s, m);
    const fs_shift_src rs = fs_shift_dword(shift + 4 * b, y, xd, H, W);
    const fs_shift_src rn = fs_shift_dword(shift + 4 * b + 2, y, xd, H, W);
    u32 v[K], w[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      v[j] = fs_shift_load(planes + fs_slot(s, j, a.P) * C, rs);
      w[j] = fs_shift_load(planes + fs_slot(s, m + j, a.P) * C, rn);
    }
    const int64_t o = b * K * C + c;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      state[o + j * C] = v[j];
      next[o + j * C] = w[j];
    }
    if (NSTEP && c == 0) fs_nstep_scalars(a, b, p, m);
  }
}

// NHWC k == 4 vector path: item i owns uint4 i of each stack
template <bool NSTEP>
__global__ void framestack_shift_nhwc4_vec_kernel(
    const u32* __restrict__ planes, const int* __restrict__ shift,
    uint4* __restrict__ state, uint4* __restrict__ next, fs_nstep_args a,
    int H, int W) {
  const int Wd = W >> 2;
  const int64_t C = (int64_t)H * Wd;
  const int64_t total = a.B * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / C;
    const int c = (int)(i - b * C);
    const int y = c / Wd, xd = c - y * Wd;
    int64_t p, s;
    int m;
    fs_shift_window<NSTEP>(a, b, p, s, m);
    const fs_shift_src rs = fs_shift_dword(shift + 4 * b, y, xd, H, W);
    const fs_shift_src rn = fs_shift_dword(shift + 4 * b + 2, y, xd, H, W);
    u32 v[4], w[4], o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = fs_shift_load(planes + fs_slot(s, j, a.P) * C, rs);
      w[j] = fs_shift_load(planes + fs_slot(s, m + j, a.P) * C, rn);
    }
    fs_transpose4(v[0], v[1], v[2], v[3], o);
    state[i] = make_uint4(o[0], o[1], o[2], o[3]);
    fs_transpose4(w[0], w[1], w[2], w[3], o);
    next[i] = make_uint4(o[0], o[1], o[2], o[3]);
    if (NSTEP && c == 0) fs_nstep_scalars(a, b, p, m);
  }
}

// scalar path: one work item = one pixel of one sample
template <bool NSTEP>
__global__ void framestack_shift_scalar_kernel(
    const u8* __restrict__ planes, const int* __restrict__ shift,
    u8* __restrict__ state, u8* __restrict__ next, fs_nstep_args a, int H,
    int W, int k, bool nhwc) {
  const int64_t HW = (int64_t)H * W;
  const int64_t total = a.B * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / HW;
    const int px = (int)(i - b * HW);
    const int y = px / W, x = px - y * W;
    int64_t p, s;
    int m;
    fs_shift_window<NSTEP>(a, b, p, s, m);
    const int* sh = shift + 4 * b;
    const int ps =
        fs_clampi(y + fs_clampi(sh[0], -(H - 1), H - 1), 0, H - 1) * W +
        fs_clampi(x + fs_clampi(sh[1], -(W - 1), W - 1), 0, W - 1);
    const int pn =
        fs_clampi(y + fs_clampi(sh[2], -(H - 1), H - 1), 0, H - 1) * W +
        fs_clampi(x + fs_clampi(sh[3], -(W - 1), W - 1), 0, W - 1);
    const int64_t o = nhwc ? i * k : b * k * HW + px;
    const int64_t step = nhwc ? 1 : HW;
    for (int j = 0; j < k; ++j) {
      state[o + j * step] = planes[fs_slot(s, j, a.P) * HW + ps];
      next[o + j * step] = planes[fs_slot(s, m + j, a.P) * HW + pn];
    }
    if (NSTEP && px == 0) fs_nstep_scalars(a, b, p, m);
  }
}

template <int K, bool NSTEP>
static void fs_launch_shift_nchw_vec(const u8* planes, const int* shift,
                                     u8* state, u8* next,
                                     const fs_nstep_args& a, int H, int W,
                                     hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL((framestack_shift_nchw_vec_kernel<K, NSTEP>),
                     dim3(ma_grid(a.B * H * (W / 4), block)), dim3(block), 0,
                     stream, (const u32*)planes, shift, (u32*)state,
                     (u32*)next, a, H, W);
}

// shared driver of the 1-step (NSTEP == false) and n-step launchers
template <bool NSTEP>
static void fs_shift_dispatch(const u8* planes, const int* shift, u8* state,
                              u8* next, const fs_nstep_args& a, int H, int W,
                              int k, bool nhwc, hipStream_t stream) {
  const int block = 256;
  const int64_t HW = (int64_t)H * W;
  // rows are 4 B aligned when the ring is and W % 4 == 0; the NHWC
  // path stores dwordx4
  const bool vec =
      (W % 4 == 0) && ((uintptr_t)planes & 3) == 0 &&
      (((uintptr_t)state | (uintptr_t)next) & 15) == 0;
  if (vec && !nhwc) {
    switch (k) {
      case 1: fs_launch_shift_nchw_vec<1, NSTEP>(planes, shift, state, next, a, H, W, stream); return;
      case 2: fs_launch_shift_nchw_vec<2, NSTEP>(planes, shift, state, next, a, H, W, stream); return;
      case 3: fs_launch_shift_nchw_vec<3, NSTEP>(planes, shift, state, next, a, H, W, stream); return;
      case 4: fs_launch_shift_nchw_vec<4, NSTEP>(planes, shift, state, next, a, H, W, stream); return;
      case 5: fs_launch_shift_nchw_vec<5, NSTEP>(planes, shift, state, next, a, H, W, stream); return;
      case 6: fs_launch_shift_nchw_vec<6, NSTEP>(planes, shift, state, next, a, H, W, stream); return;
      case 7: fs_launch_shift_nchw_vec<7, NSTEP>(planes, shift, state, next, a, H, W, stream); return;
      case 8: fs_launch_shift_nchw_vec<8, NSTEP>(planes, shift, state, next, a, H, W, stream); return;
      default: break;
    }
  }
  if (vec && nhwc && k == 4) {
    hipLaunchKernelGGL(framestack_shift_nhwc4_vec_kernel<NSTEP>,
                       dim3(ma_grid(a.B * H * (W / 4), block)), dim3(block),
                       0, stream, (const u32*)planes, shift, (uint4*)state,
                       (uint4*)next, a, H, W);
    return;
  }
  hipLaunchKernelGGL(framestack_shift_scalar_kernel<NSTEP>,
                     dim3(ma_grid(a.B * HW, block)), dim3(block), 0, stream,
                     planes, shift, state, next, a, H, W, k, nhwc);
}

// H * W < 2^30 is checked by the binding, so pixel offsets inside a
// plane and 4 * xd + dx (< 2W) stay in int32
void framestack_gather_shift_launch(const unsigned char* planes,
                                    const int64_t* base, const int* shift,
                                    unsigned char* state,
                                    unsigned char* next, int64_t B,
                                    int64_t P, int H, int W, int k,
                                    bool nhwc, hipStream_t stream) {
  if (B == 0 || H == 0 || W == 0) return;
  const fs_nstep_args a = {base,    nullptr, nullptr, nullptr, nullptr,
                           nullptr, nullptr, nullptr, B,       P,
                           0,       1,       0.0f};
  fs_shift_dispatch<false>(planes, shift, state, next, a, H, W, k, nhwc,
                           stream);
}

void framestack_gather_nstep_shift_launch(
    const unsigned char* planes, const int64_t* base, const int64_t* left,
    const float* reward, const float* terminal, const int64_t* pos,
    const int* shift, unsigned char* state, unsigned char* next,
    float* reward_n, float* terminal_n, int64_t* steps, int64_t B,
    int64_t P, int64_t T, int H, int W, int k, int n, float gamma,
    bool nhwc, hipStream_t stream) {
  if (B == 0) return;
  const fs_nstep_args a = {base,     left,       reward, terminal, pos,
                           reward_n, terminal_n, steps,  B,        P,
                           T,        n,          gamma};
  fs_shift_dispatch<true>(planes, shift, state, next, a, H, W, k, nhwc,
                          stream);
}
