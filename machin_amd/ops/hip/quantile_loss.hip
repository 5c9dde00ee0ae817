// gfx950 fused quantile-regression loss head (QR-DQN, also the loss of
// IQN and FQF): double-DQN action selection on the quantile means, the
// target-row gather, the Bellman target and the quantile Huber loss over
// all N x M pairs, one launch forward and one backward. Semantics:
// machin_amd.ops.quantile_huber_loss.
//
// The op is arithmetic-bound, unlike c51_loss.hip: N x M pairs per
// sample against (2A + 1) short rows of traffic. There is no matrix
// product in it (every pair goes through a compare, a select and a
// clamp), so MFMA does not apply; the work is plain VALU.
//
// Work split: one workgroup per sample with ceil(N / 64) waves. Lane l
// of wave w owns quantile i = 64 w + l: theta_i, tau_i, its loss partial
// and its gradient stay in registers for the whole pair loop. The M
// targets are computed once per sample into an LDS row; in the pair loop
// every lane reads the same address, a broadcast without bank conflicts,
// 16 bytes at a time. The grid strides over B with the same trip count
// in every block and `active` depends on blockIdx alone, so the barriers
// are legal.
//
// Order of every sum is fixed (j ascending per lane, butterfly across
// lanes, waves in order), so results are bit-reproducible.
//
// Every index is clamped or derived from a clamped value: no content of
// action, reward, discount or the quantile values addresses outside a
// row. NaNs propagate to loss, target and the gradient.
#include "common.h"

#define QL_MAX_QUANTILES 256
#define QL_MAX_ACTIONS 64
#define QL_PER_LANE (QL_MAX_QUANTILES / MA_WAVE)
#define QL_MAX_WAVES (QL_MAX_QUANTILES / MA_WAVE)

__device__ __forceinline__ float ql_ld(const float* p, int64_t i) {
  return p[i];
}

// bf16 as raw 16 bits, widened to fp32
__device__ __forceinline__ float ql_ld(const uint16_t* p, int64_t i) {
  return __uint_as_float((uint32_t)p[i] << 16);
}

__device__ __forceinline__ void ql_st(float* p, int64_t i, float v) {
  p[i] = v;
}

// fp32 -> bf16, round to nearest even
__device__ __forceinline__ void ql_st(uint16_t* p, int64_t i, float v) {
  uint32_t u = __float_as_uint(v);
  if (v != v) {
    p[i] = (uint16_t)((u >> 16) | 0x0040u);
  } else {
    u += 0x7fffu + ((u >> 16) & 1u);
    p[i] = (uint16_t)(u >> 16);
  }
}

// butterfly all-reduce: every lane ends with the same bits
__device__ __forceinline__ float ql_wave_sum(float v) {
#pragma unroll
  for (int off = MA_WAVE / 2; off > 0; off >>= 1)
    v += __shfl_xor(v, off, MA_WAVE);
  return v;
}

// r + g z with the product and the sum rounded separately. The
// __fmul_rn and __fadd_rn forms are plain operators to this compiler and
// contract to one fma, so contraction is switched off for the statement.
__device__ __forceinline__ float ql_target(float r, float g, float z) {
#pragma clang fp contract(off)
  const float p = g * z;
  return r + p;
}

// One pair: adds w L(u) to acc_l and w D(u) to acc_d, both still scaled
// by kappa when HUBER (the caller divides once per lane):
//   kappa L(u) = c (|u| - c / 2),  kappa D(u) = clamp(u, -kappa, kappa)
// with c = min(|u|, kappa). Without HUBER: L = |u|, D = sign(u).
template <bool HUBER>
__device__ __forceinline__ void ql_pair(float tj, float th, float tau,
                                        float one_minus_tau, float kappa,
                                        float& acc_l, float& acc_d) {
  const float u = tj - th;
  const float w = u < 0.0f ? one_minus_tau : tau;
  const float au = fabsf(u);
  float l, d;
  if (HUBER) {
    const float c = fminf(au, kappa);
    l = c * fmaf(-0.5f, c, au);
    d = fminf(fmaxf(u, -kappa), kappa);
  } else {
    l = au;
    d = u > 0.0f ? 1.0f : (u < 0.0f ? -1.0f : 0.0f);
  }
  // fminf drops a NaN from c, but l keeps it through |u|
  acc_l = fmaf(w, l, acc_l);
  acc_d = fmaf(w, d, acc_d);
}

// scale = 1 / (kappa M) when HUBER, else 1 / M.
// grad_row [B, N] receives d loss[b] / d theta[b, a_b, i].
template <typename T, bool HUBER>
__global__ void __launch_bounds__(QL_MAX_QUANTILES)
    quantile_loss_fwd_kernel(const T* __restrict__ theta,
                             const int64_t* __restrict__ action,
                             const T* __restrict__ next_online,
                             const T* __restrict__ next_target,
                             const float* __restrict__ reward,
                             const float* __restrict__ terminal,
                             const float* __restrict__ discount,  // or null
                             float discount_scalar,
                             const float* __restrict__ taus,  // or null
                             float* __restrict__ loss,
                             float* __restrict__ target,
                             int64_t* __restrict__ best_out,
                             float* __restrict__ grad_row, int64_t B, int A,
                             int N, int M, float kappa, float scale,
                             int64_t iters) {
  __shared__ float q_s[QL_MAX_ACTIONS];
  __shared__ __attribute__((aligned(16))) float t_s[QL_MAX_QUANTILES];
  __shared__ float part_s[QL_MAX_WAVES];
  const int tid = threadIdx.x;
  const int wave = tid / MA_WAVE;
  const int lane = tid % MA_WAVE;
  const int nthreads = blockDim.x;
  const int nwaves = nthreads / MA_WAVE;

  for (int64_t it = 0; it < iters; ++it) {
    const int64_t b = it * (int64_t)gridDim.x + blockIdx.x;
    const bool active = b < B;  // the same for the whole block

    // double-DQN action: the block's waves share the A rows of the
    // online net; the sum over quantiles is the mean up to 1 / M
    if (active) {
      for (int a = wave; a < A; a += nwaves) {
        const T* row = next_online + (b * A + a) * M;
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < QL_PER_LANE; ++k) {
          int j = lane + k * MA_WAVE;
          if (j < M) s += ql_ld(row, j);
        }
        s = ql_wave_sum(s);
        if (lane == 0) q_s[a] = s;
      }
    }
    __syncthreads();

    int best = 0;
    if (active) {
      // ascending a, strict >: ties go to the lowest index. A NaN sum
      // counts as maximal, as argmax has it: the first one is kept
      float best_q = -INFINITY;
      for (int a = 0; a < A; ++a) {
        float q = q_s[a];
        if (best_q == best_q && (q > best_q || q != q)) {
          best_q = q;
          best = a;
        }
      }
      // block-uniform by construction; pin it for the addressing
      best = __builtin_amdgcn_readfirstlane(best);
      best = min(max(best, 0), A - 1);

      // T_j = r + gamma (1 - terminal) z_j, once per sample; the product
      // and the sum are rounded separately, as the torch form does
      const T* row = next_target + (b * A + best) * M;
      const float r = reward[b];
      const float g =
          (discount ? discount[b] : discount_scalar) * (1.0f - terminal[b]);
      for (int j = tid; j < M; j += nthreads) {
        float tj = ql_target(r, g, ql_ld(row, j));
        t_s[j] = tj;
        target[b * M + j] = tj;
      }
    }
    __syncthreads();

    float part = 0.0f;
    if (active) {
      int64_t a_b = action[b];
      a_b = a_b < 0 ? 0 : (a_b > A - 1 ? A - 1 : a_b);
      const bool owns = tid < N;
      // lanes past N run the loop on zeros and are masked afterwards
      const float th = owns ? ql_ld(theta, (b * A + a_b) * N + tid) : 0.0f;
      float tau = 0.0f;
      if (owns)
        tau = taus ? taus[b * N + tid]
                   : (float)(2 * tid + 1) / (float)(2 * N);
      const float one_minus_tau = 1.0f - tau;
      float acc_l = 0.0f, acc_d = 0.0f;
      const int M4 = M & ~3;
      const float4* t4 = reinterpret_cast<const float4*>(t_s);
#pragma unroll 4
      for (int j = 0; j < M4; j += 4) {
        const float4 tj = t4[j >> 2];
        ql_pair<HUBER>(tj.x, th, tau, one_minus_tau, kappa, acc_l, acc_d);
        ql_pair<HUBER>(tj.y, th, tau, one_minus_tau, kappa, acc_l, acc_d);
        ql_pair<HUBER>(tj.z, th, tau, one_minus_tau, kappa, acc_l, acc_d);
        ql_pair<HUBER>(tj.w, th, tau, one_minus_tau, kappa, acc_l, acc_d);
      }
      for (int j = M4; j < M; ++j)
        ql_pair<HUBER>(t_s[j], th, tau, one_minus_tau, kappa, acc_l, acc_d);
      // clamp and sign drop a NaN that the loss partial keeps
      acc_d = acc_l != acc_l ? acc_l : acc_d;
      if (owns) {
        part = acc_l * scale;
        grad_row[b * N + tid] = -(acc_d * scale);
      }
    }
    part = ql_wave_sum(part);
    if (lane == 0) part_s[wave] = part;
    __syncthreads();

    if (active && tid == 0) {
      float total = part_s[0];
      for (int w = 1; w < nwaves; ++w) total += part_s[w];
      loss[b] = total;
      best_out[b] = best;
    }
    // the next trip writes q_s, t_s and part_s only after its own
    // barriers, which thread 0 reaches after this read
  }
}

// grad_theta, every element written: g_b * grad_row in the taken
// action's row, 0 in the others, rounded once to the input dtype.
template <typename T>
__global__ void quantile_loss_bwd_kernel(const int64_t* __restrict__ action,
                                         const float* __restrict__ grad_row,
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
    if (a == a_b) out = g[b] * grad_row[b * N + i];
    ql_st(grad, idx, out);
  }
}

template <typename T>
static void ql_fwd_dispatch(const void* theta, const int64_t* action,
                            const void* next_online, const void* next_target,
                            const float* reward, const float* terminal,
                            const float* discount, float discount_scalar,
                            const float* taus, float* loss, float* target,
                            int64_t* best, float* grad_row, int64_t B, int A,
                            int N, int M, double kappa, hipStream_t stream) {
  const bool huber = kappa > 0.0;
  const int block = MA_WAVE * ((N + MA_WAVE - 1) / MA_WAVE);
  const int grid = ma_grid(B, 1);
  const int64_t iters = (B + grid - 1) / grid;
  const float scale =
      (float)(huber ? 1.0 / (kappa * (double)M) : 1.0 / (double)M);
  auto kernel = huber ? quantile_loss_fwd_kernel<T, true>
                      : quantile_loss_fwd_kernel<T, false>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream,
                     (const T*)theta, action, (const T*)next_online,
                     (const T*)next_target, reward, terminal, discount,
                     discount_scalar, taus, loss, target, best, grad_row, B,
                     A, N, M, (float)kappa, scale, iters);
}

void quantile_loss_fwd_launch(const void* theta, const int64_t* action,
                              const void* next_online,
                              const void* next_target, const float* reward,
                              const float* terminal, const float* discount,
                              float discount_scalar, const float* taus,
                              float* loss, float* target, int64_t* best,
                              float* grad_row, int64_t B, int A, int N, int M,
                              double kappa, bool bf16, hipStream_t stream) {
  if (B == 0) return;
  if (bf16) {
    ql_fwd_dispatch<uint16_t>(theta, action, next_online, next_target,
                              reward, terminal, discount, discount_scalar,
                              taus, loss, target, best, grad_row, B, A, N, M,
                              kappa, stream);
  } else {
    ql_fwd_dispatch<float>(theta, action, next_online, next_target, reward,
                           terminal, discount, discount_scalar, taus, loss,
                           target, best, grad_row, B, A, N, M, kappa,
                           stream);
  }
}

void quantile_loss_bwd_launch(const int64_t* action, const float* grad_row,
                              const float* g, void* grad, int64_t B, int A,
                              int N, bool bf16, hipStream_t stream) {
  if (B == 0) return;
  const int block = 256;
  const int64_t total = B * A * N;
  const int grid = ma_grid(total, block);
  if (bf16) {
    hipLaunchKernelGGL(quantile_loss_bwd_kernel<uint16_t>, dim3(grid),
                       dim3(block), 0, stream, action, grad_row, g,
                       (uint16_t*)grad, total, A, N);
  } else {
    hipLaunchKernelGGL(quantile_loss_bwd_kernel<float>, dim3(grid),
                       dim3(block), 0, stream, action, grad_row, g,
                       (float*)grad, total, A, N);
  }
}
