// gfx950 whole-network fused MLP: forward, data gradient and parameter
// gradient of up to four fp32 linear layers with ReLU between them, for
// E independent networks of one shape. Semantics: machin_amd.ops.fused_mlp.
//
//   a_0 = x,  z_l = a_{l-1} W_l^T + b_l,  a_l = max(z_l, 0) (l < L),  y = z_L
//
// All three kernels run on v_mfma_f32_32x32x2_f32 (fragment layout in
// iqn_embed.hip): lane l supplies A[l % 32][l / 32] and B[l / 32][l % 32],
// and register v of a lane holds D[rho(v, l / 32)][l % 32].
//
// Forward, grid (row tiles of 32, E), 4 waves. The block's 32 rows of
// activations stay in LDS from the first layer to the last, in two
// ping-pong buffers of [32 x 256] fp32 (64 KB, so no row padding): the
// 16-byte groups of a row are XOR-swizzled by the row, which spreads the
// 32 rows that one ds_read_b128 touches at a 1024-byte stride over 32
// different groups. A layer's output columns are cut into tiles of 32
// dealt round-robin to the waves. For a chunk of 8 k, lane (row = l % 32,
// half = l / 32) reads act[row][8q + 4 half .. + 3] with one 16-byte LDS
// read and W[n0 + l % 32][8q + 4 half .. + 3] with one 16-byte global load;
// component i of both is the operand of MFMA step i, so A and B see the
// same permutation of k within the chunk and nothing is transposed.
// Weights are not staged in LDS (within a block every weight element feeds
// one wave); they stream from L2, a group of four chunks (32 k, 16 MFMAs)
// ahead of the arithmetic. Rows of W that are not 16-byte aligned
// (K % 4 != 0) take scalar loads, chosen per layer on the host. The
// epilogue adds the bias, applies ReLU, writes the tile into the other
// buffer (zero past the layer's width, which is what pads the next
// layer's k to a multiple of 8) and, when a gradient is wanted, into the
// saved [E, B, K_l] activations. The last layer goes straight to y.
//
// Backward, data path: same grid. dy's tile goes into LDS; from the last
// layer down, da_{l-1} = dz_l W_l, where the B operand W_l[n][k0 + l % 32]
// is read down a column (coalesced across the 32 lanes of k), then
// dz_{l-1} = da_{l-1} [a_{l-1} > 0] is written to the other buffer and to
// the global [E, B, K_{l-1}] buffer that the parameter kernel reads. The
// walk stops at the lowest layer whose gradient is wanted. With an x that
// the members share, each member's dx goes to its own buffer and
// fused_mlp_sum_kernel adds them in member order.
//
// Backward, parameters: one launch; blockIdx.x enumerates the 32 x 32
// tiles of every wanted dW_l through a prefix passed by value, blockIdx.y
// is the member. dW_l[n][k] = sum_b dz_l[b][n] a_{l-1}[b][k]: both
// operands come straight from global memory, coalesced across n and k.
// The four waves take interleaved chunks of 8 b and their accumulators
// are added in wave order through LDS. Tiles with k0 = 0 also produce
// db_l[n] = sum_b dz_l[b][n] from the A operands, in the same order.
//
// The prefetch distance is four chunks rather than one because one chunk's
// four MFMAs (256 cycles) do not cover an L2 round trip.
//
// No atomics, every sum has a fixed order: two calls return identical
// bits. Every global load and store is guarded by its tensor's limits.
#include "common.h"

#define FM_THREADS 256
#define FM_WAVES (FM_THREADS / MA_WAVE)
#define FM_ROWS 32    // rows (and columns) of an MFMA tile
#define FM_MAXW 256   // widest layer
#define FM_MAXL 4     // most layers
#define FM_BUF (FM_ROWS * FM_MAXW)  // floats of one activation buffer
#define FM_GROUP 4    // chunks of 8 k loaded ahead together

typedef float fm_f32x16 __attribute__((ext_vector_type(16)));

// Kernel arguments of the forward and of the data path, by value.
struct FmNet {
  const float* in;            // x [E or 1, B, k[0]] / dy [E, B, k[L]]
  float* out;                 // y [E, B, k[L]] / dx [E, B, k[0]]
  const float* w[FM_MAXL];    // [E, k[l + 1], k[l]]
  const float* b[FM_MAXL];    // [E, k[l + 1]] (forward only)
  float* sav[FM_MAXL];        // sav[l]: a_{l+1} [E, B, k[l + 1]], l < L - 1
  float* dz[FM_MAXL];         // dz[l]: dz_{l+1}, same shape (data path only)
  int64_t in_stride;          // member stride of `in`; 0 when x is shared
  int k[FM_MAXL + 1];
  int L, B;
  int vec;                    // bit l: rows of w[l] take 16-byte loads
  int save;                   // forward: write sav
  int lo;                     // data path: stop after producing layer lo
};

// Kernel arguments of the parameter kernel: the wanted layers only.
struct FmGrad {
  const float* dz[FM_MAXL];   // [E, B, n]
  const float* a[FM_MAXL];    // [E or 1, B, k]
  float* dw[FM_MAXL];         // [E, n, k]
  float* db[FM_MAXL];         // [E, n]
  int64_t a_stride[FM_MAXL];  // member stride of a; 0 when shared
  int n[FM_MAXL], k[FM_MAXL];
  int tile0[FM_MAXL + 1];     // first tile of each layer; [layers] = total
  int layers, B;
};

// row of the D operand that register v of a lane in `half` holds
__device__ __forceinline__ int fm_rho(int v, int half) {
  return 8 * (v >> 2) + 4 * half + (v & 3);
}

// LDS offset of act[row][k]: 16-byte groups swizzled by the row
__device__ __forceinline__ int fm_at(int row, int k) {
  return row * FM_MAXW + ((((k >> 2) ^ row) & 63) << 2) + (k & 3);
}

// max(z, 0) that keeps a NaN
__device__ __forceinline__ float fm_relu(float z) {
  return z <= 0.0f ? 0.0f : z;
}

// w[k .. k + 3] of a row of K elements, zero past K or when !in
template <bool VEC>
__device__ __forceinline__ float4 fm_ldw(const float* __restrict__ row,
                                         bool in, int k, int K) {
  float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (VEC) {
    // K % 4 == 0 and k % 4 == 0: k < K covers all four
    if (in && k < K) r = *reinterpret_cast<const float4*>(row + k);
  } else if (in) {
    if (k < K) r.x = row[k];
    if (k + 1 < K) r.y = row[k + 1];
    if (k + 2 < K) r.z = row[k + 2];
    if (k + 3 < K) r.w = row[k + 3];
  }
  return r;
}

// rows n .. n + 3 of column kk of W [N x K], zero past N or when !in
__device__ __forceinline__ float4 fm_ldcol(const float* __restrict__ W,
                                           bool in, int n, int kk, int N,
                                           int K) {
  float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (in) {
    const float* p = W + (int64_t)n * K + kk;
    if (n < N) r.x = p[0];
    if (n + 1 < N) r.y = p[K];
    if (n + 2 < N) r.z = p[2 * (int64_t)K];
    if (n + 3 < N) r.w = p[3 * (int64_t)K];
  }
  return r;
}

__device__ __forceinline__ void fm_mfma4(const float4& a, const float4& b,
                                         fm_f32x16& acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

// One 32 x 32 output tile: D[row][c0 + col] = sum_r act[row][r] * Bop[r][col]
// over R reduction elements, act in LDS (valid and zero-padded up to a
// multiple of 8). ROWS: Bop[r][col] = W[c0 + col][r], W is [C x R] (forward);
// otherwise Bop[r][col] = W[r][c0 + col], W is [R x C] (data path).
template <bool ROWS, bool VEC>
__device__ __forceinline__ fm_f32x16 fm_tile(const float* act,
                                             const float* __restrict__ W,
                                             int c0, int C, int R, int lane) {
  const int half = lane >> 5, j = lane & 31;
  const int c = c0 + j;
  const bool in = c < C;
  const float* wrow = W + (int64_t)(in ? c : 0) * R;  // ROWS only
  const int nq = (R + 7) >> 3;
  fm_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;

  float4 ahead[FM_GROUP];
#pragma unroll
  for (int i = 0; i < FM_GROUP; ++i) {
    const int r = 8 * i + 4 * half;
    ahead[i] = ROWS ? fm_ldw<VEC>(wrow, in, r, R)
                    : fm_ldcol(W, in, r, c, R, C);
  }
  for (int q0 = 0; q0 < nq; q0 += FM_GROUP) {
    float4 b[FM_GROUP];
#pragma unroll
    for (int i = 0; i < FM_GROUP; ++i) b[i] = ahead[i];
    if (q0 + FM_GROUP < nq) {
#pragma unroll
      for (int i = 0; i < FM_GROUP; ++i) {
        const int r = 8 * (q0 + FM_GROUP + i) + 4 * half;
        ahead[i] = ROWS ? fm_ldw<VEC>(wrow, in, r, R)
                        : fm_ldcol(W, in, r, c, R, C);
      }
    }
#pragma unroll
    for (int i = 0; i < FM_GROUP; ++i) {
      const int q = q0 + i;
      if (q < nq) {
        const float4 a = *reinterpret_cast<const float4*>(
            act + fm_at(j, 8 * q + 4 * half));
        fm_mfma4(a, b[i], acc);
      }
    }
  }
  return acc;
}

// rows r0 .. r0 + 31 of src [B x K] into an LDS buffer, zero past B and up
// to the next multiple of 8 past K
__device__ __forceinline__ void fm_fill(float* buf,
                                        const float* __restrict__ src, int r0,
                                        int B, int K) {
  const int kp = (K + 7) & ~7;
  for (int idx = threadIdx.x; idx < FM_ROWS * kp; idx += FM_THREADS) {
    const int row = idx / kp, k = idx - row * kp;
    float v = 0.0f;
    if (r0 + row < B && k < K) v = src[(int64_t)(r0 + row) * K + k];
    buf[fm_at(row, k)] = v;
  }
}

// ---------------------------------------------------------------------
// forward. grid = (row tiles, E); dynamic LDS: 2 * FM_BUF floats
// ---------------------------------------------------------------------
__global__ __launch_bounds__(FM_THREADS) void fused_mlp_fwd_kernel(FmNet p) {
  extern __shared__ __attribute__((aligned(16))) float fm_lds[];
  const int lane = threadIdx.x & (MA_WAVE - 1);
  const int wave = threadIdx.x / MA_WAVE;
  const int half = lane >> 5, j = lane & 31;
  const int r0 = blockIdx.x * FM_ROWS;
  const int64_t e = blockIdx.y;
  float* cur = fm_lds;
  float* nxt = fm_lds + FM_BUF;

  fm_fill(cur, p.in + e * p.in_stride, r0, p.B, p.k[0]);
  __syncthreads();

  for (int l = 0; l < p.L; ++l) {
    const int K = p.k[l], N = p.k[l + 1];
    const bool last = l == p.L - 1;
    const float* W = p.w[l] + e * N * K;
    const float* bias = p.b[l] + e * N;
    float* dst = nullptr;
    if (last) dst = p.out + e * p.B * N;
    else if (p.save) dst = p.sav[l] + e * p.B * N;
    const bool vec = (p.vec >> l) & 1;

    for (int n0 = wave * FM_ROWS; n0 < N; n0 += FM_WAVES * FM_ROWS) {
      const fm_f32x16 acc = vec ? fm_tile<true, true>(cur, W, n0, N, K, lane)
                                : fm_tile<true, false>(cur, W, n0, N, K, lane);
      const int n = n0 + j;
      const float bn = n < N ? bias[n] : 0.0f;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = fm_rho(v, half);
        float a = acc[v] + bn;
        if (!last) a = fm_relu(a);
        if (n >= N) a = 0.0f;
        if (!last) nxt[fm_at(row, n)] = a;
        if (dst != nullptr && r0 + row < p.B && n < N)
          dst[(int64_t)(r0 + row) * N + n] = a;
      }
    }
    __syncthreads();
    float* s = cur;
    cur = nxt;
    nxt = s;
  }
}

// ---------------------------------------------------------------------
// backward, data path. grid = (row tiles, E); dynamic LDS as the forward
// ---------------------------------------------------------------------
__global__ __launch_bounds__(FM_THREADS) void fused_mlp_bwd_data_kernel(
    FmNet p) {
  extern __shared__ __attribute__((aligned(16))) float fm_lds[];
  const int lane = threadIdx.x & (MA_WAVE - 1);
  const int wave = threadIdx.x / MA_WAVE;
  const int half = lane >> 5, j = lane & 31;
  const int r0 = blockIdx.x * FM_ROWS;
  const int64_t e = blockIdx.y;
  float* cur = fm_lds;
  float* nxt = fm_lds + FM_BUF;

  fm_fill(cur, p.in + e * p.B * p.k[p.L], r0, p.B, p.k[p.L]);
  __syncthreads();

  // layer l (1-based) turns dz_l [B x N] into da_{l-1} [B x K]
  for (int l = p.L; l > p.lo; --l) {
    const int N = p.k[l], K = p.k[l - 1];
    const bool first = l == 1;
    const float* W = p.w[l - 1] + e * N * K;
    const float* a_prev = first ? nullptr : p.sav[l - 2] + e * p.B * K;
    float* dst = (first ? p.out : p.dz[l - 2]) + e * p.B * K;

    for (int k0 = wave * FM_ROWS; k0 < K; k0 += FM_WAVES * FM_ROWS) {
      const fm_f32x16 acc = fm_tile<false, false>(cur, W, k0, K, N, lane);
      const int kk = k0 + j;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int row = fm_rho(v, half);
        const bool ok = r0 + row < p.B && kk < K;
        const int64_t at = (int64_t)(r0 + row) * K + kk;
        float g = acc[v];
        if (!first) {
          const float a = ok ? a_prev[at] : 0.0f;
          g = a > 0.0f ? g : 0.0f;
          nxt[fm_at(row, kk)] = g;
        }
        if (ok) dst[at] = g;
      }
    }
    __syncthreads();
    float* s = cur;
    cur = nxt;
    nxt = s;
  }
}

// out[i] = sum_e part[e * count + i], members added in order
__global__ void fused_mlp_sum_kernel(const float* __restrict__ part,
                                     float* __restrict__ out, int64_t count,
                                     int E) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       idx < count; idx += (int64_t)gridDim.x * blockDim.x) {
    float v = part[idx];
    for (int e = 1; e < E; ++e) v += part[(int64_t)e * count + idx];
    out[idx] = v;
  }
}

// ---------------------------------------------------------------------
// backward, parameters. grid = (tiles of every wanted layer, E)
// ---------------------------------------------------------------------
__global__ __launch_bounds__(FM_THREADS) void fused_mlp_bwd_param_kernel(
    FmGrad p) {
  __shared__ float red[FM_WAVES][16][MA_WAVE];
  __shared__ float red_b[FM_WAVES][MA_WAVE];
  const int lane = threadIdx.x & (MA_WAVE - 1);
  const int wave = threadIdx.x / MA_WAVE;
  const int half = lane >> 5, j = lane & 31;
  const int64_t e = blockIdx.y;

  int i = 0;
  while (i + 1 < p.layers && (int)blockIdx.x >= p.tile0[i + 1]) ++i;
  const int N = p.n[i], K = p.k[i], B = p.B;
  const int kt = (K + FM_ROWS - 1) / FM_ROWS;
  const int local = blockIdx.x - p.tile0[i];
  const int n0 = (local / kt) * FM_ROWS, k0 = (local % kt) * FM_ROWS;
  const float* dz = p.dz[i] + e * B * N;
  const float* a = p.a[i] + e * p.a_stride[i];
  const int n = n0 + j, kk = k0 + j;
  const bool nin = n < N, kin = kk < K;

  fm_f32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
  float dbsum = 0.0f;

  // a chunk is 8 rows of the batch; step s of it holds rows 2 s + half
  const int chunks = (B + 7) >> 3;
  float an[4], bn[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int b = 8 * wave + 2 * s + half;
    an[s] = (b < B && nin) ? dz[(int64_t)b * N + n] : 0.0f;
    bn[s] = (b < B && kin) ? a[(int64_t)b * K + kk] : 0.0f;
  }
  for (int c = wave; c < chunks; c += FM_WAVES) {
    float av[4], bv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      av[s] = an[s];
      bv[s] = bn[s];
    }
    if (c + FM_WAVES < chunks) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int b = 8 * (c + FM_WAVES) + 2 * s + half;
        an[s] = (b < B && nin) ? dz[(int64_t)b * N + n] : 0.0f;
        bn[s] = (b < B && kin) ? a[(int64_t)b * K + kk] : 0.0f;
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
      dbsum += av[s];
    }
  }

  // the four waves' accumulators, added in wave order
#pragma unroll
  for (int v = 0; v < 16; ++v) red[wave][v][lane] = acc[v];
  red_b[wave][lane] = dbsum;
  __syncthreads();
  float* dw = p.dw[i] + e * N * K;
  for (int idx = threadIdx.x; idx < 16 * MA_WAVE; idx += FM_THREADS) {
    const int v = idx >> 6, l = idx & 63;
    float sum = red[0][v][l];
#pragma unroll
    for (int w = 1; w < FM_WAVES; ++w) sum += red[w][v][l];
    const int nn = n0 + fm_rho(v, l >> 5), k = k0 + (l & 31);
    if (nn < N && k < K) dw[(int64_t)nn * K + k] = sum;
  }
  if (k0 == 0 && threadIdx.x < FM_ROWS && n0 + (int)threadIdx.x < N) {
    float sum = 0.0f;
#pragma unroll
    for (int w = 0; w < FM_WAVES; ++w)
      sum += red_b[w][threadIdx.x] + red_b[w][threadIdx.x + 32];
    p.db[i][e * N + n0 + threadIdx.x] = sum;
  }
}

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------
static bool fm_vec(const float* w, int K) {
  return K % 4 == 0 && ((uintptr_t)w & 15) == 0;
}

static FmNet fm_net(const float* const* w, const int* k, int L, int B) {
  FmNet p = {};
  for (int l = 0; l <= L; ++l) p.k[l] = k[l];
  for (int l = 0; l < L; ++l) {
    p.w[l] = w[l];
    if (fm_vec(w[l], k[l])) p.vec |= 1 << l;
  }
  p.L = L;
  p.B = B;
  return p;
}

// x [E or 1, B, k[0]] (x_stride 0: shared), w[l] [E, k[l+1], k[l]],
// b[l] [E, k[l+1]], y [E, B, k[L]]; sav[l] [E, B, k[l+1]] for l < L - 1
// when save
void fused_mlp_fwd_launch(const float* x, int64_t x_stride,
                          const float* const* w, const float* const* b,
                          float* const* sav, float* y, const int* k, int L,
                          int B, int E, bool save, hipStream_t stream) {
  FmNet p = fm_net(w, k, L, B);
  p.in = x;
  p.in_stride = x_stride;
  p.out = y;
  p.save = save;
  for (int l = 0; l < L; ++l) p.b[l] = b[l];
  for (int l = 0; save && l < L - 1; ++l) p.sav[l] = sav[l];
  hipLaunchKernelGGL(fused_mlp_fwd_kernel,
                     dim3((B + FM_ROWS - 1) / FM_ROWS, E), dim3(FM_THREADS),
                     2 * FM_BUF * sizeof(float), stream, p);
}

// dy [E, B, k[L]]; sav as the forward wrote it; dz[l] [E, B, k[l+1]] for
// lo <= l + 1 < L is written; dx_members [E, B, k[0]] when lo == 0, and
// then dx [B, k[0]] as well when x is shared (dx != nullptr). lo is the
// lowest layer (1-based) whose dz is wanted, 0 for dx; lo == L: nothing.
void fused_mlp_bwd_data_launch(const float* dy, const float* const* w,
                               float* const* sav, float* const* dz,
                               float* dx_members, float* dx, const int* k,
                               int L, int B, int E, int lo,
                               hipStream_t stream) {
  if (lo >= L) return;
  FmNet p = fm_net(w, k, L, B);
  p.in = dy;
  p.out = dx_members;
  p.lo = lo;
  for (int l = 0; l < L - 1; ++l) {
    p.sav[l] = sav[l];
    p.dz[l] = dz[l];
  }
  hipLaunchKernelGGL(fused_mlp_bwd_data_kernel,
                     dim3((B + FM_ROWS - 1) / FM_ROWS, E), dim3(FM_THREADS),
                     2 * FM_BUF * sizeof(float), stream, p);
  if (lo == 0 && dx != nullptr) {
    const int64_t count = (int64_t)B * k[0];
    hipLaunchKernelGGL(fused_mlp_sum_kernel, dim3(ma_grid(count, 256)),
                       dim3(256), 0, stream, dx_members, dx, count, E);
  }
}

// Layer l with (mask >> l) & 1: dw[l] [E, k[l+1], k[l]] and db[l]
// [E, k[l+1]] from dzs[l] [E, B, k[l+1]] (dy for the last layer) and
// acts[l] = a_l [E, B, k[l]] (x for the first, member stride x_stride).
void fused_mlp_bwd_param_launch(const float* const* dzs,
                                const float* const* acts, int64_t x_stride,
                                float* const* dw, float* const* db,
                                const int* k, int L, int B, int E, int mask,
                                hipStream_t stream) {
  FmGrad p = {};
  int tiles = 0;
  for (int l = 0; l < L; ++l) {
    if (!((mask >> l) & 1)) continue;
    const int i = p.layers++;
    p.dz[i] = dzs[l];
    p.a[i] = acts[l];
    p.a_stride[i] = l == 0 ? x_stride : (int64_t)B * k[l];
    p.dw[i] = dw[l];
    p.db[i] = db[l];
    p.n[i] = k[l + 1];
    p.k[i] = k[l];
    p.tile0[i] = tiles;
    tiles += ((k[l + 1] + FM_ROWS - 1) / FM_ROWS) *
             ((k[l] + FM_ROWS - 1) / FM_ROWS);
  }
  if (p.layers == 0) return;
  p.tile0[p.layers] = tiles;
  p.B = B;
  hipLaunchKernelGGL(fused_mlp_bwd_param_kernel, dim3(tiles, E),
                     dim3(FM_THREADS), 0, stream, p);
}
