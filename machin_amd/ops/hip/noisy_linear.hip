// gfx950 NoisyLinear (factorised Gaussian noise, Fortunato et al.):
// forward, input gradient, weight gradient and the noise fill.
// Semantics: machin_amd.ops.noisy_linear / factorised_noise_.
//
//   w[o,i] = mu[o,i] + sigma[o,i] * eps_out[o] * eps_in[i]
//
// is never stored in global memory. The forward and the input gradient
// compose one [64 x 64] tile of it in LDS per step from one read of mu
// and one of sigma (float4 loads where rows are whole aligned groups of
// 4, scalar loads otherwise: same arithmetic, same bits); the weight
// gradient writes dmu and dsigma = dmu * eps_out * eps_in from the same
// accumulator and reads neither mu nor sigma.
//
// All arithmetic is fp32 FMA from LDS-staged tiles: at replay batch
// sizes the layers are bound by the weight traffic, not by FLOPs. x and
// dy are fp32 or bf16 (widened on load), y and dx take that dtype with
// one rounding at the store.
//
// Forward and input gradient share one kernel (nl_gemm_kernel): a block
// computes a [32 batch x 64 output] tile over a contiguous slice of the
// reduction dimension. With few output tiles (B = 32) the reduction is
// split over S slices so that about two blocks per CU are in flight; each
// slice writes its partial tile to a scratch buffer and nl_reduce_kernel
// adds the slices in slice order. No atomics anywhere, every sum has a
// fixed order, so two calls return identical bits.
//
// Bounds: every global load and store is guarded by the row / column /
// reduction limit of its tensor; tiles are zero-filled past the edges.
#include "common.h"

#define NL_TB 32   // batch rows per tile
#define NL_TN 64   // output columns per tile
#define NL_KC 64   // reduction elements per step
#define NL_LD 65   // padded LDS row (odd: conflict-free column access)
#define NL_THREADS 256

__device__ __forceinline__ float nl_ld(const float* p, int64_t i) {
  return p[i];
}

// bf16 as raw 16 bits, widened to fp32
__device__ __forceinline__ float nl_ld(const uint16_t* p, int64_t i) {
  return __uint_as_float((uint32_t)p[i] << 16);
}

__device__ __forceinline__ void nl_st(float* p, int64_t i, float v) {
  p[i] = v;
}

// fp32 -> bf16, round to nearest even
__device__ __forceinline__ void nl_st(uint16_t* p, int64_t i, float v) {
  uint32_t u = __float_as_uint(v);
  if (v != v) {
    p[i] = (uint16_t)((u >> 16) | 0x0040u);
  } else {
    u += 0x7fffu + ((u >> 16) & 1u);
    p[i] = (uint16_t)(u >> 16);
  }
}

// ---------------------------------------------------------------------
// out[b, n] = sum_k a[b, k] * w(k, n)  (+ bias[n] when FWD and S == 1)
//   FWD : a = x  [B, I], k = i, n = o, K = I, N = O
//   !FWD: a = dy [B, O], k = o, n = i, K = O, N = I
// grid = (N tiles, S slices, B tiles). Slice s covers reduction steps
// [s * cps, (s + 1) * cps). With S == 1 the result goes to `out` in
// a's dtype, otherwise the fp32 partial goes to part[s, b, n].
// ---------------------------------------------------------------------
template <typename XT, bool FWD, bool VEC>
__global__ __launch_bounds__(NL_THREADS) void nl_gemm_kernel(
    const XT* __restrict__ a, const float* __restrict__ mu,
    const float* __restrict__ sigma, const float* __restrict__ bias_mu,
    const float* __restrict__ bias_sigma, const float* __restrict__ eps_in,
    const float* __restrict__ eps_out, XT* __restrict__ out,
    float* __restrict__ part, int B, int I, int O, int cps, int S) {
  __shared__ float as[NL_TB][NL_LD];
  __shared__ float ws[NL_KC][NL_LD];

  const int K = FWD ? I : O;
  const int N = FWD ? O : I;
  const int tid = threadIdx.x;
  const int lane = tid & (MA_WAVE - 1);
  const int wave = tid / MA_WAVE;
  const int n0 = blockIdx.x * NL_TN;
  const int b0 = blockIdx.z * NL_TB;
  const int s = blockIdx.y;
  const int tn = tid & 15;  // columns tn, tn+16, tn+32, tn+48
  const int tb = tid >> 4;  // rows tb, tb+16

  float acc[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0f;

  const int step_end = min((s + 1) * cps, (K + NL_KC - 1) / NL_KC);
  for (int step = s * cps; step < step_end; ++step) {
    const int k0 = step * NL_KC;
    // a tile: lanes along k (contiguous), one wave per batch row
    for (int r = wave; r < NL_TB; r += NL_THREADS / MA_WAVE) {
      const int b = b0 + r, k = k0 + lane;
      as[r][lane] =
          (b < B && k < K) ? nl_ld(a, (int64_t)b * K + k) : 0.0f;
    }
    // composed weight tile: row r is the o index, column c the i index
    // (contiguous in mu / sigma); stored as ws[k][n]
    const int o_base = FWD ? n0 : k0, i_base = FWD ? k0 : n0;
    if (VEC) {
      // I % 4 == 0 and 16-byte aligned mu / sigma: 16 lanes read one
      // 64-element row as float4, a wave reads 4 rows per instruction
      const int c = 4 * (lane & 15), i = i_base + c;
      float ei[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) ei[j] = i < I ? eps_in[i + j] : 0.0f;
      for (int r = 4 * wave + (lane >> 4); r < 64; r += NL_THREADS / 16) {
        const int o = o_base + r;
        float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f), sg = m;
        float eo = 0.0f;
        if (o < O && i < I) {
          const int64_t idx = (int64_t)o * I + i;
          m = *reinterpret_cast<const float4*>(mu + idx);
          sg = *reinterpret_cast<const float4*>(sigma + idx);
          eo = eps_out[o];
        }
        const float w[4] = {
            fmaf(sg.x, eo * ei[0], m.x), fmaf(sg.y, eo * ei[1], m.y),
            fmaf(sg.z, eo * ei[2], m.z), fmaf(sg.w, eo * ei[3], m.w)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (FWD) ws[c + j][r] = w[j]; else ws[r][c + j] = w[j];
        }
      }
    } else {
      const int i = i_base + lane;
      const float ei = i < I ? eps_in[i] : 0.0f;
      for (int r = wave; r < 64; r += NL_THREADS / MA_WAVE) {
        const int o = o_base + r;
        float w = 0.0f;
        if (o < O && i < I) {
          const int64_t idx = (int64_t)o * I + i;
          w = fmaf(sigma[idx], eps_out[o] * ei, mu[idx]);
        }
        if (FWD) ws[lane][r] = w; else ws[r][lane] = w;
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < NL_KC; ++k) {
      const float a0 = as[tb][k], a1 = as[tb + 16][k];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float w = ws[k][tn + 16 * c];
        acc[0][c] = fmaf(a0, w, acc[0][c]);
        acc[1][c] = fmaf(a1, w, acc[1][c]);
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int b = b0 + tb + 16 * r;
    if (b >= B) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int n = n0 + tn + 16 * c;
      if (n >= N) continue;
      if (S == 1) {
        float v = acc[r][c];
        if (FWD) v += fmaf(bias_sigma[n], eps_out[n], bias_mu[n]);
        nl_st(out, (int64_t)b * N + n, v);
      } else {
        part[((int64_t)s * B + b) * N + n] = acc[r][c];
      }
    }
  }
}

// out[b, n] = sum_s part[s, b, n] (+ bias[n]), slices added in order
template <typename XT, bool FWD>
__global__ void nl_reduce_kernel(const float* __restrict__ part,
                                 const float* __restrict__ bias_mu,
                                 const float* __restrict__ bias_sigma,
                                 const float* __restrict__ eps_out,
                                 XT* __restrict__ out, int64_t BN, int N,
                                 int S) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < BN; idx += (int64_t)gridDim.x * blockDim.x) {
    float v = part[idx];
#pragma unroll 8
    for (int s = 1; s < S; ++s) v += part[(int64_t)s * BN + idx];
    if (FWD) {
      const int n = (int)(idx % N);
      v += fmaf(bias_sigma[n], eps_out[n], bias_mu[n]);
    }
    nl_st(out, idx, v);
  }
}

// ---------------------------------------------------------------------
// dmu[o, i] = sum_b dy[b, o] x[b, i], dsigma = dmu * eps_out[o] * eps_in[i],
// dbias_mu[o] = sum_b dy[b, o], dbias_sigma = dbias_mu * eps_out[o].
// grid = (I tiles of 64, O tiles of 32). A block walks the whole batch
// in steps of 32 rows, so each of dmu / dsigma is written exactly once;
// the blocks of the first I tile also sum the bias gradients.
// ---------------------------------------------------------------------
#define NL_WO 32
#define NL_WI 64
#define NL_WB 32

template <typename XT>
__global__ __launch_bounds__(NL_THREADS) void nl_bwd_weight_kernel(
    const XT* __restrict__ dy, const XT* __restrict__ x,
    const float* __restrict__ eps_in, const float* __restrict__ eps_out,
    float* __restrict__ dmu, float* __restrict__ dsigma,
    float* __restrict__ dbias_mu, float* __restrict__ dbias_sigma, int B,
    int I, int O) {
  __shared__ float dys[NL_WB][NL_WO + 1];
  __shared__ __attribute__((aligned(16))) float xs[NL_WB][NL_WI];

  const int tid = threadIdx.x;
  const int lane = tid & (MA_WAVE - 1);
  const int wave = tid / MA_WAVE;
  const int i0 = blockIdx.x * NL_WI;
  const int o0 = blockIdx.y * NL_WO;
  const int tx = tid & 15;  // columns 4 tx .. 4 tx + 3
  const int ty = tid >> 4;  // rows ty, ty + 16
  const bool do_bias = blockIdx.x == 0 && tid < NL_WO;

  float acc[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0f;
  float bsum = 0.0f;

  for (int bb = 0; bb < B; bb += NL_WB) {
    for (int r = wave; r < NL_WB; r += NL_THREADS / MA_WAVE) {
      const int b = bb + r, i = i0 + lane;
      xs[r][lane] = (b < B && i < I) ? nl_ld(x, (int64_t)b * I + i) : 0.0f;
    }
    // dy tile: half a wave per batch row
    for (int r = tid >> 5; r < NL_WB; r += NL_THREADS / 32) {
      const int b = bb + r, o = o0 + (tid & 31);
      dys[r][tid & 31] =
          (b < B && o < O) ? nl_ld(dy, (int64_t)b * O + o) : 0.0f;
    }
    __syncthreads();
#pragma unroll 8
    for (int b = 0; b < NL_WB; ++b) {
      const float d0 = dys[b][ty], d1 = dys[b][ty + 16];
      const float4 xv = *reinterpret_cast<const float4*>(&xs[b][4 * tx]);
      acc[0][0] = fmaf(d0, xv.x, acc[0][0]);
      acc[0][1] = fmaf(d0, xv.y, acc[0][1]);
      acc[0][2] = fmaf(d0, xv.z, acc[0][2]);
      acc[0][3] = fmaf(d0, xv.w, acc[0][3]);
      acc[1][0] = fmaf(d1, xv.x, acc[1][0]);
      acc[1][1] = fmaf(d1, xv.y, acc[1][1]);
      acc[1][2] = fmaf(d1, xv.z, acc[1][2]);
      acc[1][3] = fmaf(d1, xv.w, acc[1][3]);
    }
    if (do_bias) {
#pragma unroll 8
      for (int b = 0; b < NL_WB; ++b) bsum += dys[b][tid];
    }
    __syncthreads();
  }

  const int ib = i0 + 4 * tx;
  float ei[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) ei[c] = (ib + c < I) ? eps_in[ib + c] : 0.0f;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int o = o0 + ty + 16 * r;
    if (o >= O) continue;
    const float eo = eps_out[o];
    const int64_t row = (int64_t)o * I;
    float g[4], gs[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      g[c] = acc[r][c];
      gs[c] = g[c] * (eo * ei[c]);
    }
    if ((I & 3) == 0 && ib + 3 < I) {
      // rows are 16-byte aligned when I is a multiple of 4
      *reinterpret_cast<float4*>(dmu + row + ib) =
          make_float4(g[0], g[1], g[2], g[3]);
      *reinterpret_cast<float4*>(dsigma + row + ib) =
          make_float4(gs[0], gs[1], gs[2], gs[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (ib + c < I) {
          dmu[row + ib + c] = g[c];
          dsigma[row + ib + c] = gs[c];
        }
      }
    }
  }
  if (do_bias) {
    const int o = o0 + tid;
    if (o < O) {
      dbias_mu[o] = bsum;
      dbias_sigma[o] = bsum * eps_out[o];
    }
  }
}

// ---------------------------------------------------------------------
// buf[i] = f(z_i), f(z) = sign(z) sqrt(|z|), z_i ~ N(0, 1) from Philox
// keyed by (seed, element index i, offset). One launch fills a layer's
// eps_in and eps_out, which are views of one buffer.
// ---------------------------------------------------------------------
__global__ void factorised_noise_kernel(float* __restrict__ buf, int64_t n,
                                        uint64_t seed, uint64_t offset) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t r[4];
    ma_philox4(seed, (uint64_t)i, offset, r);
    float z, unused;
    ma_box_muller(ma_u32_to_uniform(r[0]), ma_u32_to_uniform(r[1]), &z,
                  &unused);
    buf[i] = copysignf(sqrtf(fabsf(z)), z);
  }
}

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------

// Number of reduction slices for a [B, N] output reduced over K: enough
// for about two blocks per CU (512), at least one step per slice.
// Returns steps per slice in *cps.
int noisy_linear_slices(int64_t B, int64_t N, int64_t K, int* cps) {
  const int64_t tiles =
      ((B + NL_TB - 1) / NL_TB) * ((N + NL_TN - 1) / NL_TN);
  const int64_t steps = (K + NL_KC - 1) / NL_KC;
  int64_t want = (512 + tiles - 1) / tiles;
  if (want > steps) want = steps;
  if (want < 1) want = 1;
  const int64_t per = (steps + want - 1) / want;
  *cps = (int)per;
  return (int)((steps + per - 1) / per);
}

template <typename XT, bool FWD>
static void nl_gemm_launch(const void* a, const float* mu, const float* sigma,
                           const float* bias_mu, const float* bias_sigma,
                           const float* eps_in, const float* eps_out,
                           void* out, float* part, int B, int I, int O,
                           int cps, int S, hipStream_t stream) {
  const int N = FWD ? O : I;
  dim3 grid((N + NL_TN - 1) / NL_TN, S, (B + NL_TB - 1) / NL_TB);
  // float4 weight loads need whole, 16-byte aligned groups of 4 per row
  const bool vec = (I % 4 == 0) && ((uintptr_t)mu % 16 == 0) &&
                   ((uintptr_t)sigma % 16 == 0);
  if (vec) {
    hipLaunchKernelGGL((nl_gemm_kernel<XT, FWD, true>), grid,
                       dim3(NL_THREADS), 0, stream, (const XT*)a, mu, sigma,
                       bias_mu, bias_sigma, eps_in, eps_out, (XT*)out, part,
                       B, I, O, cps, S);
  } else {
    hipLaunchKernelGGL((nl_gemm_kernel<XT, FWD, false>), grid,
                       dim3(NL_THREADS), 0, stream, (const XT*)a, mu, sigma,
                       bias_mu, bias_sigma, eps_in, eps_out, (XT*)out, part,
                       B, I, O, cps, S);
  }
  if (S > 1) {
    const int64_t BN = (int64_t)B * N;
    hipLaunchKernelGGL((nl_reduce_kernel<XT, FWD>), dim3(ma_grid(BN, 256)),
                       dim3(256), 0, stream, part, bias_mu, bias_sigma,
                       eps_out, (XT*)out, BN, N, S);
  }
}

// part: fp32 [S, B, O] scratch, used when S > 1
void noisy_linear_fwd_launch(const void* x, const float* mu,
                             const float* sigma, const float* bias_mu,
                             const float* bias_sigma, const float* eps_in,
                             const float* eps_out, void* y, float* part,
                             int B, int I, int O, int cps, int S, bool bf16,
                             hipStream_t stream) {
  if (bf16) {
    nl_gemm_launch<uint16_t, true>(x, mu, sigma, bias_mu, bias_sigma, eps_in,
                                   eps_out, y, part, B, I, O, cps, S, stream);
  } else {
    nl_gemm_launch<float, true>(x, mu, sigma, bias_mu, bias_sigma, eps_in,
                                eps_out, y, part, B, I, O, cps, S, stream);
  }
}

// part: fp32 [S, B, I] scratch, used when S > 1
void noisy_linear_bwd_input_launch(const void* dy, const float* mu,
                                   const float* sigma, const float* eps_in,
                                   const float* eps_out, void* dx,
                                   float* part, int B, int I, int O, int cps,
                                   int S, bool bf16, hipStream_t stream) {
  if (bf16) {
    nl_gemm_launch<uint16_t, false>(dy, mu, sigma, nullptr, nullptr, eps_in,
                                    eps_out, dx, part, B, I, O, cps, S,
                                    stream);
  } else {
    nl_gemm_launch<float, false>(dy, mu, sigma, nullptr, nullptr, eps_in,
                                 eps_out, dx, part, B, I, O, cps, S, stream);
  }
}

void noisy_linear_bwd_weight_launch(const void* dy, const void* x,
                                    const float* eps_in, const float* eps_out,
                                    float* dmu, float* dsigma,
                                    float* dbias_mu, float* dbias_sigma,
                                    int B, int I, int O, bool bf16,
                                    hipStream_t stream) {
  dim3 grid((I + NL_WI - 1) / NL_WI, (O + NL_WO - 1) / NL_WO);
  if (bf16) {
    hipLaunchKernelGGL(nl_bwd_weight_kernel<uint16_t>, grid,
                       dim3(NL_THREADS), 0, stream, (const uint16_t*)dy,
                       (const uint16_t*)x, eps_in, eps_out, dmu, dsigma,
                       dbias_mu, dbias_sigma, B, I, O);
  } else {
    hipLaunchKernelGGL(nl_bwd_weight_kernel<float>, grid, dim3(NL_THREADS),
                       0, stream, (const float*)dy, (const float*)x, eps_in,
                       eps_out, dmu, dsigma, dbias_mu, dbias_sigma, B, I, O);
  }
}

void factorised_noise_launch(float* buf, int64_t n, uint64_t seed,
                             uint64_t offset, hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(factorised_noise_kernel, dim3(ma_grid(n, block)),
                     dim3(block), 0, stream, buf, n, seed, offset);
}
