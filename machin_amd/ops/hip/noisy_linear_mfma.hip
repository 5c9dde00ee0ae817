// gfx950 NoisyLinear for bf16 x and many rows: forward, input gradient
// and weight gradient on the bf16 matrix unit.
// Semantics: machin_amd.ops.noisy_linear / ops._NoisyLinearMFMA.
//
//   w[o,i] = mu[o,i] + sigma[o,i] * eps_out[o] * eps_in[i]
//
// is composed in fp32 exactly as in noisy_linear.hip and never stored in
// global memory. For the matrix unit it is split into two bf16 halves,
//
//   hi = bf16_rne(w),  lo = bf16_rne(w - float(hi))   (subtraction exact)
//
// so that |w - hi - lo| <= 2^-16 |w|, and y / dx are
// sum a * hi + sum a * lo: one a fragment feeds two MFMAs, each half has
// its own fp32 accumulator and the two are added once at the end. The
// weight gradient has bf16 operands on both sides (dy and x), its
// products are exact in fp32 and it takes one MFMA per fragment.
//
// Instruction: v_mfma_f32_16x16x32_bf16. Fragment layout (pinned by
// mfma_probe): lane l holds A[m = l & 15][k = 8 (l >> 4) + j] and
// B[k = 8 (l >> 4) + j][n = l & 15], j = 0..7, and gets
// D[4 (l >> 4) + reg][l & 15]. Both operands therefore want "8
// consecutive k of one row / column" per lane, and every LDS tile here
// is kept in that fragment order: a [64 x 32] tile is 4 sub-tiles of
// 16 rows, a sub-tile is 64 slots of 16 bytes, slot
// (kq << 4) | (row & 15) holds k = 8 kq .. 8 kq + 7 of that row. A
// fragment is then one conflict-free ds_read_b128 at slot == lane.
//
// Work split: a block of 4 waves owns a [64 x 64] output tile, a wave a
// [32 x 32] quarter of it (2 x 2 MFMA tiles), and the reduction runs in
// steps of 64 (two MFMA k-steps). 64 x 64 rather than 128 x 128 so that
// the 2048 x 512 forward of the IQN head is 256 blocks, one per CU,
// without splitting the reduction: no partial buffer, no second kernel.
// The global loads of step s + 1 are issued into registers before the
// MFMAs of step s and written to LDS after them.
//
// Where the reduction index is contiguous in memory (x, dy as the a
// operand; mu / sigma in the forward, k = i) a thread loads its 8 k as
// one 16-byte (a) or two float4 (mu, sigma) loads when the row length
// allows it, scalar loads otherwise. Where it is strided (mu / sigma
// for dx, k = o; dy and x in the weight gradient, k = row) a thread
// loads 8 rows of one column, lanes along the column index, so each
// load instruction is one contiguous line per wave and the transpose
// happens in registers: no transposed LDS image, no ds_read_tr.
//
// No atomics, every sum has a fixed order: two calls return equal bits.
// Bounds: every global load and store is guarded by the row / column /
// reduction limit of its tensor; tiles are zero-filled past the edges.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define NM_T 64          // output tile rows and columns
#define NM_KC 64         // reduction elements per step
#define NM_KS (NM_KC / 32)  // MFMA k-steps per step
#define NM_THREADS 256

// fragment-order tile: [k-step][sub-tile of 16 rows][slot]
typedef bf16x8 nm_tile[NM_KS][NM_T / 16][64];

__device__ __forceinline__ int nm_slot(int row, int kq) {
  return (kq << 4) | (row & 15);
}

__device__ __forceinline__ bf16x8 nm_zero8() {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.0f;
  return v;
}

// One wave's [32 x 32] quarter over one step: acc += A * B
__device__ __forceinline__ void nm_mma(const nm_tile& as, const nm_tile& bs,
                                       int wm, int wn, int lane,
                                       f32x4 acc[2][2]) {
#pragma unroll
  for (int ks = 0; ks < NM_KS; ++ks) {
    bf16x8 af[2], bf[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      af[t] = as[ks][2 * wm + t][lane];
      bf[t] = bs[ks][2 * wn + t][lane];
    }
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
      for (int n2 = 0; n2 < 2; ++n2)
        acc[m2][n2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[m2], bf[n2], acc[m2][n2], 0, 0, 0);
  }
}

// ---------------------------------------------------------------------
// out[r, n] = sum_k a[r, k] * w(k, n)  (+ bias[n] when FWD)
//   FWD : a = x  [R, I], k = i, n = o, K = I, N = O
//   !FWD: a = dy [R, O], k = o, n = i, K = O, N = I
// grid = (row tiles, N tiles): neighbouring blocks share a weight tile.
// avec: rows of a are whole 16-byte aligned groups of 8; wvec (FWD):
// rows of mu / sigma are whole 16-byte aligned groups of 4.
// ---------------------------------------------------------------------
template <bool FWD>
__global__ __launch_bounds__(NM_THREADS) void nm_gemm_kernel(
    const __bf16* __restrict__ a, const float* __restrict__ mu,
    const float* __restrict__ sigma, const float* __restrict__ bias_mu,
    const float* __restrict__ bias_sigma, const float* __restrict__ eps_in,
    const float* __restrict__ eps_out, __bf16* __restrict__ out, int R, int I,
    int O, int avec, int wvec) {
  __shared__ nm_tile as, wh, wl;

  const int K = FWD ? I : O;
  const int N = FWD ? O : I;
  const int tid = threadIdx.x;
  const int lane = tid & (MA_WAVE - 1);
  const int wave = tid / MA_WAVE;
  const int wm = wave >> 1, wn = wave & 1;
  const int r0 = blockIdx.x * NM_T;
  const int n0 = blockIdx.y * NM_T;

  // a loader: row ar, k-group akq (8 contiguous k)
  const int ar = tid >> 2, akq = tid & 3;
  const int64_t arow = (int64_t)(r0 + ar) * K;
  const bool a_ok = r0 + ar < R;
  // w loader: output column wc, k-group wkq. FWD: k = i is contiguous, 4
  // threads cover 32 i of one o. !FWD: k = o is strided, lanes run along i.
  const int wc = FWD ? tid >> 2 : tid & 63;
  const int wkq = FWD ? tid & 3 : tid >> 6;
  const bool w_ok = n0 + wc < N;
  // the noise factor of this thread's column: eps_out[o] or eps_in[i]
  const float e_col = w_ok ? (FWD ? eps_out : eps_in)[n0 + wc] : 0.0f;

  bf16x8 pa[NM_KS];
  float pm[NM_KS][8], ps[NM_KS][8], pe[NM_KS][8];

  auto load = [&](int k0) {
#pragma unroll
    for (int ks = 0; ks < NM_KS; ++ks) {
      const int ka = k0 + 32 * ks + 8 * akq;
      pa[ks] = nm_zero8();
      if (a_ok && ka < K) {
        if (avec) {
          pa[ks] = *reinterpret_cast<const bf16x8*>(a + arow + ka);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (ka + j < K) pa[ks][j] = a[arow + ka + j];
        }
      }
      const int kw = k0 + 32 * ks + 8 * wkq;
#pragma unroll
      for (int j = 0; j < 8; ++j) pm[ks][j] = ps[ks][j] = pe[ks][j] = 0.0f;
      if (FWD) {
        if (w_ok && kw < I) {
          const int64_t idx = (int64_t)(n0 + wc) * I + kw;
          if (wvec) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              if (kw + 4 * h < I) {
                const float4 m =
                    *reinterpret_cast<const float4*>(mu + idx + 4 * h);
                const float4 s =
                    *reinterpret_cast<const float4*>(sigma + idx + 4 * h);
                const float4 e =
                    *reinterpret_cast<const float4*>(eps_in + kw + 4 * h);
                pm[ks][4 * h] = m.x, pm[ks][4 * h + 1] = m.y;
                pm[ks][4 * h + 2] = m.z, pm[ks][4 * h + 3] = m.w;
                ps[ks][4 * h] = s.x, ps[ks][4 * h + 1] = s.y;
                ps[ks][4 * h + 2] = s.z, ps[ks][4 * h + 3] = s.w;
                pe[ks][4 * h] = e.x, pe[ks][4 * h + 1] = e.y;
                pe[ks][4 * h + 2] = e.z, pe[ks][4 * h + 3] = e.w;
              }
            }
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              if (kw + j < I) {
                pm[ks][j] = mu[idx + j];
                ps[ks][j] = sigma[idx + j];
                pe[ks][j] = eps_in[kw + j];
              }
            }
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (w_ok && kw + j < O) {
            const int64_t idx = (int64_t)(kw + j) * I + n0 + wc;
            pm[ks][j] = mu[idx];
            ps[ks][j] = sigma[idx];
            pe[ks][j] = eps_out[kw + j];
          }
        }
      }
    }
  };

  f32x4 acc_hi[2][2], acc_lo[2][2];
#pragma unroll
  for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
    for (int n2 = 0; n2 < 2; ++n2)
      acc_hi[m2][n2] = acc_lo[m2][n2] = (f32x4)(0.0f);

  const int steps = (K + NM_KC - 1) / NM_KC;
  load(0);
  for (int step = 0; step < steps; ++step) {
#pragma unroll
    for (int ks = 0; ks < NM_KS; ++ks) {
      as[ks][ar >> 4][nm_slot(ar, akq)] = pa[ks];
      bf16x8 hi, lo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // eps_out * eps_in, as in noisy_linear.hip
        const float w = fmaf(ps[ks][j], e_col * pe[ks][j], pm[ks][j]);
        hi[j] = (__bf16)w;
        lo[j] = (__bf16)(w - (float)hi[j]);
      }
      wh[ks][wc >> 4][nm_slot(wc, wkq)] = hi;
      wl[ks][wc >> 4][nm_slot(wc, wkq)] = lo;
    }
    __syncthreads();
    if (step + 1 < steps) load((step + 1) * NM_KC);
    nm_mma(as, wh, wm, wn, lane, acc_hi);
    nm_mma(as, wl, wm, wn, lane, acc_lo);
    __syncthreads();
  }

#pragma unroll
  for (int n2 = 0; n2 < 2; ++n2) {
    const int n = n0 + 32 * wn + 16 * n2 + (lane & 15);
    if (n >= N) continue;
    float bias = 0.0f;
    if (FWD) bias = fmaf(bias_sigma[n], eps_out[n], bias_mu[n]);
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int r = r0 + 32 * wm + 16 * m2 + 4 * (lane >> 4) + reg;
        if (r >= R) continue;
        float v = acc_hi[m2][n2][reg] + acc_lo[m2][n2][reg];
        if (FWD) v += bias;
        out[(int64_t)r * N + n] = (__bf16)v;
      }
    }
  }
}

// ---------------------------------------------------------------------
// dmu[o, i] = sum_r dy[r, o] x[r, i], dsigma = dmu * eps_out[o] * eps_in[i],
// dbias_mu[o] = sum_r dy[r, o], dbias_sigma = dbias_mu * eps_out[o].
// grid = (I tiles, O tiles). A block walks all rows in steps of 64, so
// dmu / dsigma are written exactly once; the blocks of the first I tile
// also sum the bias gradients, in row order, from the dy tile in LDS.
// The reduction index (row) is strided in both operands: a thread loads
// 8 rows of one column of each.
// ---------------------------------------------------------------------
__global__ __launch_bounds__(NM_THREADS) void nm_wgrad_kernel(
    const __bf16* __restrict__ dy, const __bf16* __restrict__ x,
    const float* __restrict__ eps_in, const float* __restrict__ eps_out,
    float* __restrict__ dmu, float* __restrict__ dsigma,
    float* __restrict__ dbias_mu, float* __restrict__ dbias_sigma, int R,
    int I, int O) {
  __shared__ nm_tile ds, xs;

  const int tid = threadIdx.x;
  const int lane = tid & (MA_WAVE - 1);
  const int wave = tid / MA_WAVE;
  const int wm = wave >> 1, wn = wave & 1;
  const int i0 = blockIdx.x * NM_T;
  const int o0 = blockIdx.y * NM_T;
  const int c = tid & 63, kq = tid >> 6;
  const bool d_ok = o0 + c < O, x_ok = i0 + c < I;
  const bool do_bias = blockIdx.x == 0 && tid < NM_T;

  bf16x8 pd[NM_KS], px[NM_KS];
  auto load = [&](int k0) {
#pragma unroll
    for (int ks = 0; ks < NM_KS; ++ks) {
      pd[ks] = nm_zero8();
      px[ks] = nm_zero8();
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = k0 + 32 * ks + 8 * kq + j;
        if (r < R) {
          if (d_ok) pd[ks][j] = dy[(int64_t)r * O + o0 + c];
          if (x_ok) px[ks][j] = x[(int64_t)r * I + i0 + c];
        }
      }
    }
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
    for (int n2 = 0; n2 < 2; ++n2) acc[m2][n2] = (f32x4)(0.0f);
  float bsum = 0.0f;

  const int steps = (R + NM_KC - 1) / NM_KC;
  load(0);
  for (int step = 0; step < steps; ++step) {
#pragma unroll
    for (int ks = 0; ks < NM_KS; ++ks) {
      ds[ks][c >> 4][nm_slot(c, kq)] = pd[ks];
      xs[ks][c >> 4][nm_slot(c, kq)] = px[ks];
    }
    __syncthreads();
    if (step + 1 < steps) load((step + 1) * NM_KC);
    nm_mma(ds, xs, wm, wn, lane, acc);
    if (do_bias) {
#pragma unroll
      for (int ks = 0; ks < NM_KS; ++ks)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bf16x8 v = ds[ks][tid >> 4][nm_slot(tid, q)];
#pragma unroll
          for (int j = 0; j < 8; ++j) bsum += (float)v[j];
        }
    }
    __syncthreads();
  }

#pragma unroll
  for (int n2 = 0; n2 < 2; ++n2) {
    const int i = i0 + 32 * wn + 16 * n2 + (lane & 15);
    if (i >= I) continue;
    const float ei = eps_in[i];
#pragma unroll
    for (int m2 = 0; m2 < 2; ++m2) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int o = o0 + 32 * wm + 16 * m2 + 4 * (lane >> 4) + reg;
        if (o >= O) continue;
        const float g = acc[m2][n2][reg];
        const int64_t idx = (int64_t)o * I + i;
        dmu[idx] = g;
        dsigma[idx] = g * (eps_out[o] * ei);
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
// host side
// ---------------------------------------------------------------------
template <bool FWD>
static void nm_gemm_launch(const void* a, const float* mu, const float* sigma,
                           const float* bias_mu, const float* bias_sigma,
                           const float* eps_in, const float* eps_out,
                           void* out, int R, int I, int O,
                           hipStream_t stream) {
  const int K = FWD ? I : O, N = FWD ? O : I;
  dim3 grid((R + NM_T - 1) / NM_T, (N + NM_T - 1) / NM_T);
  const int avec = (K % 8 == 0) && ((uintptr_t)a % 16 == 0);
  const int wvec = (I % 4 == 0) && ((uintptr_t)mu % 16 == 0) &&
                   ((uintptr_t)sigma % 16 == 0) &&
                   ((uintptr_t)eps_in % 16 == 0);
  hipLaunchKernelGGL((nm_gemm_kernel<FWD>), grid, dim3(NM_THREADS), 0, stream,
                     (const __bf16*)a, mu, sigma, bias_mu, bias_sigma, eps_in,
                     eps_out, (__bf16*)out, R, I, O, avec, wvec);
}

// x [R, I] bf16 -> y [R, O] bf16
void noisy_linear_mfma_fwd_launch(const void* x, const float* mu,
                                  const float* sigma, const float* bias_mu,
                                  const float* bias_sigma,
                                  const float* eps_in, const float* eps_out,
                                  void* y, int R, int I, int O,
                                  hipStream_t stream) {
  nm_gemm_launch<true>(x, mu, sigma, bias_mu, bias_sigma, eps_in, eps_out, y,
                       R, I, O, stream);
}

// dy [R, O] bf16 -> dx [R, I] bf16
void noisy_linear_mfma_bwd_input_launch(const void* dy, const float* mu,
                                        const float* sigma,
                                        const float* eps_in,
                                        const float* eps_out, void* dx, int R,
                                        int I, int O, hipStream_t stream) {
  nm_gemm_launch<false>(dy, mu, sigma, nullptr, nullptr, eps_in, eps_out, dx,
                        R, I, O, stream);
}

void noisy_linear_mfma_bwd_weight_launch(const void* dy, const void* x,
                                         const float* eps_in,
                                         const float* eps_out, float* dmu,
                                         float* dsigma, float* dbias_mu,
                                         float* dbias_sigma, int R, int I,
                                         int O, hipStream_t stream) {
  dim3 grid((I + NM_T - 1) / NM_T, (O + NM_T - 1) / NM_T);
  hipLaunchKernelGGL(nm_wgrad_kernel, grid, dim3(NM_THREADS), 0, stream,
                     (const __bf16*)dy, (const __bf16*)x, eps_in, eps_out, dmu,
                     dsigma, dbias_mu, dbias_sigma, R, I, O);
}
