// gfx950 fused C51 loss head (RAINBOW): double-DQN action selection,
// target-row gather, categorical projection with a per-sample discount
// and the cross-entropy of the taken row, one launch forward and one
// backward. Semantics: machin_amd.ops.c51_loss.
//
// Forward follows projection.hip: one wavefront per sample, lanes
// across atoms (N <= 256, so at most 4 atoms per lane, kept in
// registers), the projected row accumulated in a per-wave LDS row with
// LDS atomics (no global atomics, guide §6 G12) and read back for the
// loss reduction and the coalesced store. Every wave runs the same trip
// count, so __syncthreads() is legal; inactive waves skip only the
// work. Rows of N atoms start at arbitrary element offsets (N = 51), so
// loads stay scalar per lane; the op is launch-latency-bound at replay
// batch sizes.
//
// Every index is clamped or derived from a clamped value: no content of
// action, reward, discount or the distributions addresses outside a
// row. NaNs propagate to the outputs.
#include "common.h"

#define C51_MAX_ATOMS 256
#define C51_WAVES_PER_BLOCK 4
#define C51_PER_LANE (C51_MAX_ATOMS / MA_WAVE)

__device__ __forceinline__ float c51_ld(const float* p, int64_t i) {
  return p[i];
}

// bf16 as raw 16 bits, widened to fp32
__device__ __forceinline__ float c51_ld(const uint16_t* p, int64_t i) {
  return __uint_as_float((uint32_t)p[i] << 16);
}

__device__ __forceinline__ void c51_st(float* p, int64_t i, float v) {
  p[i] = v;
}

// fp32 -> bf16, round to nearest even
__device__ __forceinline__ void c51_st(uint16_t* p, int64_t i, float v) {
  uint32_t u = __float_as_uint(v);
  if (v != v) {
    p[i] = (uint16_t)((u >> 16) | 0x0040u);
  } else {
    u += 0x7fffu + ((u >> 16) & 1u);
    p[i] = (uint16_t)(u >> 16);
  }
}

// butterfly all-reduce: every lane ends with the same bits
__device__ __forceinline__ float c51_wave_sum(float v) {
#pragma unroll
  for (int off = MA_WAVE / 2; off > 0; off >>= 1)
    v += __shfl_xor(v, off, MA_WAVE);
  return v;
}

// max that keeps a NaN (fmaxf would drop it)
__device__ __forceinline__ float c51_max(float a, float b) {
  return (a != a || a > b) ? a : b;
}

__device__ __forceinline__ float c51_wave_max(float v) {
#pragma unroll
  for (int off = MA_WAVE / 2; off > 0; off >>= 1)
    v = c51_max(v, __shfl_xor(v, off, MA_WAVE));
  return v;
}

// Loads one row of N atoms into x[] (lane l holds atoms l, l+64, ...;
// slots past N are left untouched and never read).
// LOGITS: returns the row's log-sum-exp, so exp(x - lse) is the softmax.
// Otherwise returns 0.
template <typename T, bool LOGITS>
__device__ __forceinline__ float c51_load_row(const T* __restrict__ row,
                                              int N, int lane,
                                              float x[C51_PER_LANE]) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < C51_PER_LANE; ++k) {
    int i = lane + k * MA_WAVE;
    if (i < N) {
      x[k] = c51_ld(row, i);
      m = c51_max(m, x[k]);
    }
  }
  if (!LOGITS) return 0.0f;
  m = c51_wave_max(m);
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < C51_PER_LANE; ++k) {
    int i = lane + k * MA_WAVE;
    if (i < N) s += expf(x[k] - m);
  }
  return m + logf(c51_wave_sum(s));
}

template <typename T, bool LOGITS>
__global__ void __launch_bounds__(MA_WAVE* C51_WAVES_PER_BLOCK)
    c51_loss_fwd_kernel(const T* __restrict__ dist,
                        const int64_t* __restrict__ action,
                        const T* __restrict__ next_online,
                        const T* __restrict__ next_target,
                        const float* __restrict__ reward,
                        const float* __restrict__ terminal,
                        const float* __restrict__ discount,  // or null
                        float discount_scalar, float* __restrict__ loss,
                        float* __restrict__ proj,
                        int64_t* __restrict__ best_out,
                        float* __restrict__ lse_out,
                        float* __restrict__ s_out, int64_t B, int A, int N,
                        float v_min, float v_max, float delta_z,
                        int64_t iters) {
  __shared__ float acc[C51_WAVES_PER_BLOCK][C51_MAX_ATOMS];
  const int wave = threadIdx.x / MA_WAVE;
  const int lane = threadIdx.x % MA_WAVE;
  const int64_t row_stride = (int64_t)gridDim.x * C51_WAVES_PER_BLOCK;

  for (int64_t it = 0; it < iters; ++it) {
    const int64_t b =
        it * row_stride + (int64_t)blockIdx.x * C51_WAVES_PER_BLOCK + wave;
    const bool active = b < B;
    float x[C51_PER_LANE];
    int best = 0;

    if (active) {
#pragma unroll
      for (int k = 0; k < C51_PER_LANE; ++k) {
        int i = lane + k * MA_WAVE;
        if (i < N) acc[wave][i] = 0.0f;
      }
    }
    __syncthreads();

    if (active) {
      // double-DQN action: lowest a with maximal expected value
      float best_q = -INFINITY;
      for (int a = 0; a < A; ++a) {
        float lse = c51_load_row<T, LOGITS>(
            next_online + (b * A + a) * N, N, lane, x);
        float qz = 0.0f;
#pragma unroll
        for (int k = 0; k < C51_PER_LANE; ++k) {
          int i = lane + k * MA_WAVE;
          if (i < N) {
            float p = LOGITS ? expf(x[k] - lse) : x[k];
            qz += p * (v_min + delta_z * (float)i);
          }
        }
        float q = c51_wave_sum(qz);
        if (q > best_q) {
          best_q = q;
          best = a;
        }
      }
      // wave-uniform by construction; pin it for the addressing
      best = __builtin_amdgcn_readfirstlane(best);
      best = min(max(best, 0), A - 1);

      // projection of the target net's row for that action
      float lse = c51_load_row<T, LOGITS>(
          next_target + (b * A + best) * N, N, lane, x);
      const float r = reward[b];
      const float g =
          (discount ? discount[b] : discount_scalar) * (1.0f - terminal[b]);
      const float top = (float)(N - 1);
#pragma unroll
      for (int k = 0; k < C51_PER_LANE; ++k) {
        int i = lane + k * MA_WAVE;
        if (i < N) {
          float p = LOGITS ? expf(x[k] - lse) : x[k];
          float tz = r + g * (v_min + delta_z * (float)i);
          if (tz != tz) p = tz;  // NaN target: NaN mass, bin 0
          tz = fminf(fmaxf(tz, v_min), v_max);
          float pos = (tz - v_min) / delta_z;
          float lo_f = floorf(pos), hi_f = ceilf(pos);
          float w_lo = lo_f == hi_f ? 1.0f : hi_f - pos;
          float w_hi = pos - lo_f;
          // clamp as floats first (converting a huge value is
          // undefined), then as integers
          int lo = (int)fminf(fmaxf(lo_f, 0.0f), top);
          int hi = (int)fminf(fmaxf(hi_f, 0.0f), top);
          lo = min(max(lo, 0), N - 1);
          hi = min(max(hi, 0), N - 1);
          atomicAdd(&acc[wave][lo], p * w_lo);
          if (lo_f != hi_f) atomicAdd(&acc[wave][hi], p * w_hi);
        }
      }
    }
    __syncthreads();

    if (active) {
      // cross-entropy of the taken action's row against the projection
      int64_t a_b = action[b];
      a_b = a_b < 0 ? 0 : (a_b > A - 1 ? A - 1 : a_b);
      float lse = c51_load_row<T, LOGITS>(dist + (b * A + a_b) * N, N,
                                          lane, x);
      float ce = 0.0f, psum = 0.0f;
#pragma unroll
      for (int k = 0; k < C51_PER_LANE; ++k) {
        int i = lane + k * MA_WAVE;
        if (i < N) {
          float pj = acc[wave][i];
          proj[b * N + i] = pj;
          float logp =
              LOGITS ? x[k] - lse : logf(x[k] < 1e-8f ? 1e-8f : x[k]);
          ce -= pj * logp;
          psum += pj;
        }
      }
      ce = c51_wave_sum(ce);
      psum = c51_wave_sum(psum);
      if (lane == 0) {
        loss[b] = ce;
        best_out[b] = best;
        lse_out[b] = lse;
        s_out[b] = psum;
      }
    }
    __syncthreads();
  }
}

// grad_dist, every element written (rows of untaken actions get 0):
//   probabilities: -g * proj / dist where dist >= 1e-8, else 0
//   logits:         g * (exp(dist - lse) * S - proj)
template <typename T, bool LOGITS>
__global__ void c51_loss_bwd_kernel(const T* __restrict__ dist,
                                    const int64_t* __restrict__ action,
                                    const float* __restrict__ proj,
                                    const float* __restrict__ lse,
                                    const float* __restrict__ s_sum,
                                    const float* __restrict__ g,
                                    T* __restrict__ grad, int64_t total,
                                    int A, int N) {
  const int64_t AN = (int64_t)A * N;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = idx / AN;
    const int rem = (int)(idx - b * AN);
    const int a = rem / N;
    const int i = rem - a * N;
    int64_t a_b = action[b];
    a_b = a_b < 0 ? 0 : (a_b > A - 1 ? A - 1 : a_b);
    float out = 0.0f;
    if (a == a_b) {
      const float x = c51_ld(dist, idx);
      const float pj = proj[b * N + i];
      if (LOGITS) {
        out = g[b] * (expf(x - lse[b]) * s_sum[b] - pj);
      } else if (x >= 1e-8f) {
        out = -g[b] * pj / x;
      }
    }
    c51_st(grad, idx, out);
  }
}

template <typename T>
static void c51_fwd_dispatch(const void* dist, const int64_t* action,
                             const void* next_online,
                             const void* next_target, const float* reward,
                             const float* terminal, const float* discount,
                             float discount_scalar, float* loss,
                             float* proj, int64_t* best, float* lse,
                             float* s_sum, int64_t B, int A, int N,
                             float v_min, float v_max, bool from_logits,
                             hipStream_t stream) {
  const float delta_z = (v_max - v_min) / (float)(N - 1);
  const int block = MA_WAVE * C51_WAVES_PER_BLOCK;
  int64_t row_groups = (B + C51_WAVES_PER_BLOCK - 1) / C51_WAVES_PER_BLOCK;
  int grid = ma_grid(row_groups, 1);
  int64_t rows_per_pass = (int64_t)grid * C51_WAVES_PER_BLOCK;
  int64_t iters = (B + rows_per_pass - 1) / rows_per_pass;
  auto kernel = from_logits ? c51_loss_fwd_kernel<T, true>
                            : c51_loss_fwd_kernel<T, false>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream,
                     (const T*)dist, action, (const T*)next_online,
                     (const T*)next_target, reward, terminal, discount,
                     discount_scalar, loss, proj, best, lse, s_sum, B, A, N,
                     v_min, v_max, delta_z, iters);
}

void c51_loss_fwd_launch(const void* dist, const int64_t* action,
                         const void* next_online, const void* next_target,
                         const float* reward, const float* terminal,
                         const float* discount, float discount_scalar,
                         float* loss, float* proj, int64_t* best,
                         float* lse, float* s_sum, int64_t B, int A, int N,
                         float v_min, float v_max, bool bf16,
                         bool from_logits, hipStream_t stream) {
  if (B == 0) return;
  if (bf16) {
    c51_fwd_dispatch<uint16_t>(dist, action, next_online, next_target,
                               reward, terminal, discount, discount_scalar,
                               loss, proj, best, lse, s_sum, B, A, N, v_min,
                               v_max, from_logits, stream);
  } else {
    c51_fwd_dispatch<float>(dist, action, next_online, next_target, reward,
                            terminal, discount, discount_scalar, loss, proj,
                            best, lse, s_sum, B, A, N, v_min, v_max,
                            from_logits, stream);
  }
}

template <typename T>
static void c51_bwd_dispatch(const void* dist, const int64_t* action,
                             const float* proj, const float* lse,
                             const float* s_sum, const float* g, void* grad,
                             int64_t B, int A, int N, bool from_logits,
                             hipStream_t stream) {
  const int block = 256;
  const int64_t total = B * A * N;
  auto kernel = from_logits ? c51_loss_bwd_kernel<T, true>
                            : c51_loss_bwd_kernel<T, false>;
  hipLaunchKernelGGL(kernel, dim3(ma_grid(total, block)), dim3(block), 0,
                     stream, (const T*)dist, action, proj, lse, s_sum, g,
                     (T*)grad, total, A, N);
}

void c51_loss_bwd_launch(const void* dist, const int64_t* action,
                         const float* proj, const float* lse,
                         const float* s_sum, const float* g, void* grad,
                         int64_t B, int A, int N, bool bf16,
                         bool from_logits, hipStream_t stream) {
  if (B == 0) return;
  if (bf16) {
    c51_bwd_dispatch<uint16_t>(dist, action, proj, lse, s_sum, g, grad, B,
                               A, N, from_logits, stream);
  } else {
    c51_bwd_dispatch<float>(dist, action, proj, lse, s_sum, g, grad, B, A,
                            N, from_logits, stream);
  }
}
