// Fused bias + ReLU epilogue for the MIOpen convs of the Atari stack
// (conv2 / conv3), on the NHWC bf16 [R, C] view of a channels-last
// activation (R = N*H*W rows, C channels, C % 8 == 0).
//
// Why: after a bias-free MIOpen conv the eager path runs a broadcast
// bias add_ and then an in-place ReLU — two read+write passes over the
// activation — and in backward a threshold_backward pass followed by a
// bias-gradient reduction that re-reads the gradient. All four are
// pure HBM streaming with no arithmetic to speak of. Here:
//
// - bias_relu_: ONE in-place pass, y = relu(bf16(float(y) +
//   float(bf16(bias[c])))) — the exact rounding sequence of autocast's
//   bf16 bias, ATen's fp32-opmath add_ and ReLU, so results are
//   bit-identical to the unfused path.
// - bias_relu_bwd: ONE pass reads gy and the saved activation y,
//   writes gx = y > 0 ? gy : 0 and accumulates the per-channel sum of
//   gx. The sum is deterministic: fp32 per-thread partials over a fixed
//   row assignment, a fixed-order LDS reduction per block, per-block
//   partials in a small buffer and a fixed-order finishing kernel (no
//   float atomics: the bias gradient must not change from run to run).
//
// - bias_relu_flat / bias_relu_flat_bwd: the same pair for the LAST
//   conv, whose output feeds nn.Flatten. Flatten of a channels-last
//   activation is an NHWC -> NCHW copy forward, and its backward hands
//   an NCHW gradient to a channels-last consumer (a strided
//   threshold_backward or one more copy). The forward variant writes
//   relu(y + bias) directly as the NCHW-flat [N, C*HW] matrix (one
//   per-sample transpose through LDS); the backward variant reads the
//   NCHW-flat gradient and activation, both in the same layout, and
//   writes the NHWC gx through the same LDS tile. The fc weight keeps
//   its meaning: the flat matrix is exactly what Flatten produced.
//
// All kernels move 16 B per lane (guide §6 G13) and grid-stride over
// a capped grid (G11).
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 ba_bf16x8;

#define BA_BLOCK 256

__global__ __launch_bounds__(BA_BLOCK)
void bias_relu_kernel(__bf16* __restrict__ y,
                      const float* __restrict__ bias, int64_t n_vec,
                      int C) {
  const int64_t stride = (int64_t)gridDim.x * BA_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * BA_BLOCK + threadIdx.x;
       i < n_vec; i += stride) {
    const int c0 = (int)((i * 8) % C);
    ba_bf16x8 v = *(const ba_bf16x8*)(y + i * 8);
    const float4 b_lo = *(const float4*)(bias + c0);
    const float4 b_hi = *(const float4*)(bias + c0 + 4);
    const float b[8] = {b_lo.x, b_lo.y, b_lo.z, b_lo.w,
                        b_hi.x, b_hi.y, b_hi.z, b_hi.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      __bf16 s = (__bf16)((float)v[j] + (float)(__bf16)b[j]);
      // !(s <= 0) keeps NaN, as ATen's relu does
      v[j] = !((float)s <= 0.0f) ? s : (__bf16)0.0f;
    }
    *(ba_bf16x8*)(y + i * 8) = v;
  }
}

// Row assignment (fixed by R, C and the grid alone): V = C/8 lanes
// cover one row, a block covers RP = 256/V rows per pass and owns the
// contiguous rows [blockIdx*rows_per_block, +rows_per_block); lane
// (rl, cg) = (tid / V, tid % V) walks rows rl, rl+RP, ... of that span
// and keeps 8 fp32 column sums.
__global__ __launch_bounds__(BA_BLOCK)
void bias_relu_bwd_kernel(const __bf16* __restrict__ gy,
                          const __bf16* __restrict__ y,
                          __bf16* __restrict__ gx,
                          float* __restrict__ partial,  // [grid][C]
                          int64_t R, int C, int64_t rows_per_block) {
  __shared__ float s_part[BA_BLOCK * 8];
  const int tid = threadIdx.x;
  const int V = C / 8;
  const int RP = BA_BLOCK / V;
  const int rl = tid / V, cg = tid % V;
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r_end = min(r_begin + rows_per_block, R);

  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0f;

  if (rl < RP) {
    for (int64_t r = r_begin + rl; r < r_end; r += RP) {
      const int64_t off = r * C + cg * 8;
      ba_bf16x8 g = *(const ba_bf16x8*)(gy + off);
      const ba_bf16x8 a = *(const ba_bf16x8*)(y + off);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // ATen threshold_backward: x <= 0 ? 0 : grad
        g[j] = ((float)a[j] <= 0.0f) ? (__bf16)0.0f : g[j];
        acc[j] += (float)g[j];
      }
      *(ba_bf16x8*)(gx + off) = g;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) s_part[tid * 8 + j] = acc[j];
  __syncthreads();
  // channel c = cg*8 + j: sum the RP row-lanes in index order
  for (int c = tid; c < C; c += BA_BLOCK) {
    const int ccg = c >> 3, j = c & 7;
    float s = 0.0f;
    for (int q = 0; q < RP; ++q) s += s_part[(q * V + ccg) * 8 + j];
    partial[(int64_t)blockIdx.x * C + c] = s;
  }
}

// Finishing pass, one block: channel c is summed by P = 256/C (at
// least 1) lanes, lane p taking blocks p, p+P, ... in order; the P
// lane sums are then added in index order. Result rounded to bf16 (what
// the eager bf16 reduction with fp32 accumulation returns) and stored
// as fp32.
__global__ __launch_bounds__(BA_BLOCK)
void bias_relu_bwd_finish_kernel(const float* __restrict__ partial,
                                 float* __restrict__ out, int n_blocks,
                                 int C) {
  __shared__ float s_sum[BA_BLOCK];
  const int tid = threadIdx.x;
  const int P = C < BA_BLOCK ? BA_BLOCK / C : 1;
  const int span = P == 1 ? BA_BLOCK : C;  // channels per sweep
  const int p = tid / span;
  for (int c_base = 0; c_base < C; c_base += span) {
    const int c = c_base + tid % span;
    float s = 0.0f;
    if (c < C && p < P) {
#pragma unroll 8
      for (int b = p; b < n_blocks; b += P) {
        s += partial[(int64_t)b * C + c];
      }
    }
    s_sum[tid] = s;
    __syncthreads();
    if (p == 0 && c < C) {
      float tot = 0.0f;
      for (int q = 0; q < P; ++q) tot += s_sum[q * span + tid];
      out[c] = (float)(__bf16)tot;
    }
    __syncthreads();
  }
}

// ---- NCHW-flat variants (conv -> Flatten) -----------------------------
// One sample at a time per block: its [HW][C] tile is C*HW bf16 in
// dynamic LDS, laid out as the NCHW-flat row (index c*HW + hw).
// C*HW % 8 == 0 keeps every sample's flat row 16 B aligned.
__global__ __launch_bounds__(BA_BLOCK)
void bias_relu_flat_kernel(const __bf16* __restrict__ y,   // [N][HW][C]
                           const float* __restrict__ bias,
                           __bf16* __restrict__ out,       // [N][C*HW]
                           int64_t N, int C, int HW) {
  extern __shared__ __attribute__((aligned(16))) __bf16 s_tile[];
  const int tid = threadIdx.x;
  const int V = C / 8;
  const int n_vec = HW * V;  // 16 B pieces per sample, either layout
  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    const __bf16* src = y + n * (int64_t)n_vec * 8;
    for (int v = tid; v < n_vec; v += BA_BLOCK) {
      const int hw = v / V, c0 = (v % V) * 8;
      const ba_bf16x8 a = *(const ba_bf16x8*)(src + (int64_t)v * 8);
      const float4 b_lo = *(const float4*)(bias + c0);
      const float4 b_hi = *(const float4*)(bias + c0 + 4);
      const float b[8] = {b_lo.x, b_lo.y, b_lo.z, b_lo.w,
                          b_hi.x, b_hi.y, b_hi.z, b_hi.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        __bf16 s = (__bf16)((float)a[j] + (float)(__bf16)b[j]);
        s_tile[(c0 + j) * HW + hw] =
            !((float)s <= 0.0f) ? s : (__bf16)0.0f;
      }
    }
    __syncthreads();
    __bf16* dst = out + n * (int64_t)n_vec * 8;
    for (int v = tid; v < n_vec; v += BA_BLOCK) {
      *(ba_bf16x8*)(dst + (int64_t)v * 8) =
          *(const ba_bf16x8*)(s_tile + v * 8);
    }
    __syncthreads();
  }
}

// Row assignment: block b owns samples b, b+grid, ...; inside a sample
// lane (rl, cg) = (tid / V, tid % V) takes pixels rl, rl+RP, ... .
__global__ __launch_bounds__(BA_BLOCK)
void bias_relu_flat_bwd_kernel(const __bf16* __restrict__ gy,  // [N][C*HW]
                               const __bf16* __restrict__ y,   // [N][C*HW]
                               __bf16* __restrict__ gx,        // [N][HW][C]
                               float* __restrict__ partial,    // [grid][C]
                               int64_t N, int C, int HW) {
  // C*HW bf16, and at least BA_BLOCK*8 floats for the final reduction
  extern __shared__ __attribute__((aligned(16))) __bf16 s_tile[];
  const int tid = threadIdx.x;
  const int V = C / 8;
  const int RP = BA_BLOCK / V;
  const int rl = tid / V, cg = tid % V;
  const int n_vec = HW * V;

  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0f;

  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    const int64_t base = n * (int64_t)n_vec * 8;
    for (int v = tid; v < n_vec; v += BA_BLOCK) {
      ba_bf16x8 g = *(const ba_bf16x8*)(gy + base + (int64_t)v * 8);
      const ba_bf16x8 a = *(const ba_bf16x8*)(y + base + (int64_t)v * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        g[j] = ((float)a[j] <= 0.0f) ? (__bf16)0.0f : g[j];
      }
      *(ba_bf16x8*)(s_tile + v * 8) = g;
    }
    __syncthreads();
    if (rl < RP) {
      for (int hw = rl; hw < HW; hw += RP) {
        ba_bf16x8 g;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          g[j] = s_tile[(cg * 8 + j) * HW + hw];
          acc[j] += (float)g[j];
        }
        *(ba_bf16x8*)(gx + base + ((int64_t)hw * V + cg) * 8) = g;
      }
    }
    __syncthreads();
  }
  float* s_part = (float*)s_tile;
#pragma unroll
  for (int j = 0; j < 8; ++j) s_part[tid * 8 + j] = acc[j];
  __syncthreads();
  for (int c = tid; c < C; c += BA_BLOCK) {
    const int ccg = c >> 3, j = c & 7;
    float s = 0.0f;
    for (int q = 0; q < RP; ++q) s += s_part[(q * V + ccg) * 8 + j];
    partial[(int64_t)blockIdx.x * C + c] = s;
  }
}

static size_t flat_lds_bytes(int C, int HW) {
  size_t tile = (size_t)C * HW * sizeof(__bf16);
  size_t red = (size_t)BA_BLOCK * 8 * sizeof(float);
  return tile > red ? tile : red;
}

int64_t bias_relu_flat_blocks(int64_t N) {
  return N < 2048 ? (N < 1 ? 1 : N) : 2048;
}

void bias_relu_flat_launch(const void* y, const float* bias, void* out,
                           int64_t N, int C, int HW, hipStream_t stream) {
  if (N == 0) return;
  hipLaunchKernelGGL(bias_relu_flat_kernel,
                     dim3((unsigned)bias_relu_flat_blocks(N)),
                     dim3(BA_BLOCK), flat_lds_bytes(C, HW), stream,
                     (const __bf16*)y, bias, (__bf16*)out, N, C, HW);
  HIP_CHECK(hipGetLastError());
}

void bias_relu_launch(void* y, const float* bias, int64_t R, int C,
                      hipStream_t stream) {
  const int64_t n_vec = R * C / 8;
  if (n_vec == 0) return;
  hipLaunchKernelGGL(bias_relu_kernel, dim3(ma_grid(n_vec, BA_BLOCK)),
                     dim3(BA_BLOCK), 0, stream, (__bf16*)y, bias, n_vec,
                     C);
  HIP_CHECK(hipGetLastError());
}

// number of per-block partial rows bias_relu_bwd_launch will write
// (the caller sizes the workspace with it); depends on R and C only
int64_t bias_relu_bwd_blocks(int64_t R, int C) {
  const int RP = BA_BLOCK / (C / 8);
  int64_t blocks = (R + RP - 1) / RP;  // one pass per block at most
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return blocks;
}

void bias_relu_bwd_launch(const void* gy, const void* y, void* gx,
                          float* partial, float* grad_bias, int64_t R,
                          int C, hipStream_t stream) {
  const int RP = BA_BLOCK / (C / 8);
  const int64_t blocks = bias_relu_bwd_blocks(R, C);
  int64_t rows_per_block = (R + blocks - 1) / blocks;
  rows_per_block = (rows_per_block + RP - 1) / RP * RP;
  if (rows_per_block < RP) rows_per_block = RP;
  // every block writes its partial row, also one whose span is empty
  hipLaunchKernelGGL(bias_relu_bwd_kernel, dim3((unsigned)blocks),
                     dim3(BA_BLOCK), 0, stream, (const __bf16*)gy,
                     (const __bf16*)y, (__bf16*)gx, partial, R, C,
                     rows_per_block);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(bias_relu_bwd_finish_kernel, dim3(1), dim3(BA_BLOCK),
                     0, stream, partial, grad_bias, (int)blocks, C);
  HIP_CHECK(hipGetLastError());
}

void bias_relu_flat_bwd_launch(const void* gy, const void* y, void* gx,
                               float* partial, float* grad_bias,
                               int64_t N, int C, int HW,
                               hipStream_t stream) {
  const int64_t blocks = bias_relu_flat_blocks(N);
  hipLaunchKernelGGL(bias_relu_flat_bwd_kernel, dim3((unsigned)blocks),
                     dim3(BA_BLOCK), flat_lds_bytes(C, HW), stream,
                     (const __bf16*)gy, (const __bf16*)y, (__bf16*)gx,
                     partial, N, C, HW);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(bias_relu_bwd_finish_kernel, dim3(1), dim3(BA_BLOCK),
                     0, stream, partial, grad_bias, (int)blocks, C);
  HIP_CHECK(hipGetLastError());
}
