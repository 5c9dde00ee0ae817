// gfx950 fused weight-gradient kernel for the Atari stem conv
// (Conv2d(C_in=4, C_out=32, kernel 8x8, stride 4) on 84x84 frames).
//
// Why hand-written: the weight gradient of this layer is a skinny
// reduction GEMM dW[32,256] = dy^T[32,K] @ im2col(x)[K,256] with
// K = batch*400 (16.4M at bench batch 40960). MIOpen/CK pick kernels
// that run it at ~2% MFMA efficiency (2.5-5.4 ms/step measured,
// profiles/impala_bench_kernel_trace_r01.md). The op is HBM-bound in
// principle: dy (1.05 GB bf16) + x (1.16 GB u8, read ONCE as u8 and
// dequantized in-register) ≈ 2.2 GB -> ~0.4 ms at 6 TB/s.
//
// Design (guide §3, §5):
// - mfma_f32_16x16x32_bf16 tiles; output 32x256 = 2x16 tiles of
//   16x16; 4 waves per workgroup, each owns (M-tile, 8 N-tiles),
//   32 f32 accumulator registers per lane.
// - split-K: each workgroup reduces its K-slice and atomicAdd's the
//   32x256 fp32 partial (atomics are a rounding-free fp32 add; the
//   slab is tiny so contention is negligible — guide §6 G12).
// - x rows are assembled from the NHWC u8 frame tensor: one im2col
//   row = 8 segments of 32 contiguous bytes; 256 threads stage a
//   16-row chunk into LDS as bf16 (dequant scale fused into the
//   u8->bf16 conversion).
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define CONV1_CIN 4
#define CONV1_COUT 32
#define CONV1_KSZ 8
#define CONV1_STRIDE 4
#define CONV1_OHW 20          // output spatial (84-8)/4+1
#define CONV1_POS (CONV1_OHW * CONV1_OHW)       // 400 positions
#define CONV1_N (CONV1_KSZ * CONV1_KSZ * CONV1_CIN)  // 256 patch size
#define KC 32  // k-rows per chunk: one full MFMA K-step (16x16x32)

__device__ __forceinline__ __bf16 u8_bf16(unsigned char v, float scale) {
  return (__bf16)((float)v * scale);
}

// dy: [K, 32] bf16 row-major (K = B*400, NHWC conv output layout)
// frames: [B, 84, 84, 4] u8 (NHWC)
// out: [32, 256] fp32, PRE-ZEROED, atomicAdd target
__global__ __launch_bounds__(256)
void conv1_wrw_kernel(const __bf16* __restrict__ dy,
                      const unsigned char* __restrict__ frames,
                      float* __restrict__ out,
                      float* __restrict__ b_out, int64_t K,
                      int64_t k_per_wg, float scale) {
  __shared__ __bf16 lds[KC * CONV1_COUT + KC * CONV1_N];  // dy | x
  __bf16* s_dy = lds;                    // [KC][32]
  __bf16* s_x = lds + KC * CONV1_COUT;   // [KC][256]

  const int tid = threadIdx.x;
  const int wave = tid / MA_WAVE;  // 0..3
  const int lane = tid % MA_WAVE;
  const int mt = wave & 1;         // M-tile (0..1): rows mt*16..mt*16+15
  const int ng = wave >> 1;        // N-group (0..1): tiles ng*8..ng*8+7

  f32x4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = (f32x4)(0.0f);
  float bias_acc = 0.0f;

  const int64_t k_begin = (int64_t)blockIdx.x * k_per_wg;
  const int64_t k_end = min(k_begin + k_per_wg, K);

  for (int64_t kc = k_begin; kc < k_end; kc += KC) {
    // ---- stage dy chunk: 32 rows x 32 bf16 (64B/row) --------------
    // threads 0..127: each loads 16B (8 bf16)
    if (tid < 128) {
      int row = tid >> 2;        // 0..31
      int seg = tid & 3;         // 0..3 (8 bf16 each)
      int64_t kk = kc + row;
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.0f;
      if (kk < k_end) {
        v = *(const bf16x8*)(dy + kk * CONV1_COUT + seg * 8);
      }
      *(bf16x8*)(s_dy + row * CONV1_COUT + seg * 8) = v;
    }
    // ---- stage x chunk: 32 rows x 256 bf16 from u8 patches --------
    // each im2col row: 8 segments of 32 u8; 256 segments total;
    // 256 threads -> each converts one full 32-byte segment
    {
      int row = tid >> 3;        // k-row 0..31
      int r = tid & 7;           // patch row 0..7
      int64_t kk = kc + row;
      bf16x8 q0, q1, q2, q3;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        q0[j] = (__bf16)0.0f;
        q1[j] = (__bf16)0.0f;
        q2[j] = (__bf16)0.0f;
        q3[j] = (__bf16)0.0f;
      }
      if (kk < k_end) {
        int64_t b = kk / CONV1_POS;
        int pos = (int)(kk % CONV1_POS);
        int oh = pos / CONV1_OHW, ow = pos % CONV1_OHW;
        const unsigned char* src =
            frames
            + ((b * 84 + (int64_t)oh * CONV1_STRIDE + r) * 84
               + (int64_t)ow * CONV1_STRIDE) * CONV1_CIN;
        uint4 raw0 = *(const uint4*)src;
        uint4 raw1 = *(const uint4*)(src + 16);
        unsigned int words[8] = {raw0.x, raw0.y, raw0.z, raw0.w,
                                 raw1.x, raw1.y, raw1.z, raw1.w};
#pragma unroll
        for (int w = 0; w < 2; ++w) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            q0[w * 4 + j] = u8_bf16((words[w] >> (8 * j)) & 0xFF, scale);
            q1[w * 4 + j] =
                u8_bf16((words[w + 2] >> (8 * j)) & 0xFF, scale);
            q2[w * 4 + j] =
                u8_bf16((words[w + 4] >> (8 * j)) & 0xFF, scale);
            q3[w * 4 + j] =
                u8_bf16((words[w + 6] >> (8 * j)) & 0xFF, scale);
          }
        }
      }
      bf16x8* dst = (bf16x8*)(s_x + row * CONV1_N + r * 32);
      dst[0] = q0;
      dst[1] = q1;
      dst[2] = q2;
      dst[3] = q3;
    }
    __syncthreads();

    // ---- fused bias: wave 0 lanes 0..31 sum dy columns (dy is
    // already in LDS; saves a separate 1 GB reduction pass) ---------
    if (wave == 0 && lane < CONV1_COUT) {
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        bias_acc += (float)s_dy[k * CONV1_COUT + lane];
      }
    }

    // ---- MFMA: A[m,k]=dy[k, mt*16+m] (transposed read), B[k,n]=x --
    // A fragment (16x16x32): lane holds m=lane%16, k=(lane/16)*8+j
    bf16x8 a_frag;
    {
      int m = lane & 15;
      int k0 = (lane >> 4) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a_frag[j] = s_dy[(k0 + j) * CONV1_COUT + mt * 16 + m];
      }
    }
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      int n0 = (ng * 8 + nt) * 16;
      bf16x8 b_frag;
      int n = lane & 15;
      int k0 = (lane >> 4) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        b_frag[j] = s_x[(k0 + j) * CONV1_N + n0 + n];
      }
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_frag, b_frag, acc[nt], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue: atomicAdd partials (C/D map: col=lane&15,
  // row=(lane>>4)*4+reg) ------------------------------------------
  if (wave == 0 && lane < CONV1_COUT) {
    atomicAdd(&b_out[lane], bias_acc);
  }
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) {
    int col = (ng * 8 + nt) * 16 + (lane & 15);
    int row_base = mt * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      atomicAdd(&out[(row_base + reg) * CONV1_N + col], acc[nt][reg]);
    }
  }
}

// reorder [32][r*32+c*4+ci] fp32 -> conv weight grad [32][4][8][8]
__global__ void conv1_wrw_reorder_kernel(const float* __restrict__ in,
                                         float* __restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= CONV1_COUT * CONV1_N) return;
  int co = i / CONV1_N;
  int rem = i % CONV1_N;
  int r = rem / 32;
  int c = (rem % 32) / CONV1_CIN;
  int ci = rem % CONV1_CIN;
  out[((co * CONV1_CIN + ci) * CONV1_KSZ + r) * CONV1_KSZ + c] =
      in[i];
}

__global__ void conv1_wrw_v2_kernel(const __bf16*, const unsigned char*,
                                    float*, float*, int64_t, int64_t,
                                    float);
__global__ void conv1_fwd_v2_kernel(const unsigned char*, const __bf16*,
                                    const float*, __bf16*, int64_t, float);
__global__ void conv1_wrw_v3_kernel(const __bf16*, const unsigned char*,
                                    float*, float*, int64_t, int64_t,
                                    float);
__global__ void conv1_fwd_v3_kernel(const unsigned char*, const __bf16*,
                                    const float*, __bf16*, int64_t, float);
bool conv1_fwd_v4_launch(const unsigned char*, const void*, const float*,
                         void*, unsigned int*, bool, int64_t, float,
                         hipStream_t);
bool conv1_wrw_v4_launch(const void*, const unsigned int*,
                         const unsigned char*, float*, float*, int64_t,
                         int64_t, float, hipStream_t);

void conv1_wrw_launch(const void* dy, const unsigned char* frames,
                      float* scratch, float* grad_w, float* grad_b,
                      int64_t K, float scale, hipStream_t stream) {
  HIP_CHECK(hipMemsetAsync(scratch, 0,
                           CONV1_COUT * CONV1_N * sizeof(float), stream));
  HIP_CHECK(hipMemsetAsync(grad_b, 0, CONV1_COUT * sizeof(float),
                           stream));
  // split-K: target ~2048 workgroups (8 XCDs x 32 CUs x 8 blocks)
  int64_t target_wg = 2048;
  if (const char* e = getenv("MACHIN_CONV1_WG")) target_wg = atol(e);
  const char* ver = getenv("MACHIN_CONV1_V");
  int v = ver ? atoi(ver) : 4;
  if (v != 1 && v != 2 && v != 3 &&
      conv1_wrw_v4_launch(dy, nullptr, frames, scratch, grad_b, K,
                          target_wg, scale, stream)) {
    hipLaunchKernelGGL(conv1_wrw_reorder_kernel,
                       dim3((CONV1_COUT * CONV1_N + 255) / 256), dim3(256),
                       0, stream, scratch, grad_w);
    HIP_CHECK(hipGetLastError());
    return;
  }
  int64_t chunk = (v == 1 || v == 2) ? 32 : 64;
  if (target_wg < 1) target_wg = 1;
  int64_t k_per_wg = (K + target_wg - 1) / target_wg;
  k_per_wg = ((k_per_wg + chunk - 1) / chunk) * chunk;
  if (k_per_wg < chunk) k_per_wg = chunk;
  int grid = (int)((K + k_per_wg - 1) / k_per_wg);
  if (v == 1) {
    hipLaunchKernelGGL(conv1_wrw_kernel, dim3(grid), dim3(256), 0, stream,
                       (const __bf16*)dy, frames, scratch, grad_b, K,
                       k_per_wg, scale);
  } else if (v == 2) {
    hipLaunchKernelGGL(conv1_wrw_v2_kernel, dim3(grid), dim3(256), 0,
                       stream, (const __bf16*)dy, frames, scratch, grad_b,
                       K, k_per_wg, scale);
  } else {
    hipLaunchKernelGGL(conv1_wrw_v3_kernel, dim3(grid), dim3(256), 0,
                       stream, (const __bf16*)dy, frames, scratch, grad_b,
                       K, k_per_wg, scale);
  }
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(conv1_wrw_reorder_kernel,
                     dim3((CONV1_COUT * CONV1_N + 255) / 256), dim3(256),
                     0, stream, scratch, grad_w);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------
// layout probe: one mfma_f32_16x16x32_bf16 tile, D = A[16,32] @ B[32,16]
// with the fragment maps assumed above. Used by tests to pin the
// lane->element mapping before trusting the conv kernel.
// ---------------------------------------------------------------------
__global__ void mfma_probe_kernel(const __bf16* __restrict__ A,
                                  const __bf16* __restrict__ B,
                                  float* __restrict__ D) {
  int lane = threadIdx.x;
  bf16x8 a_frag, b_frag;
  int m = lane & 15;
  int k0 = (lane >> 4) * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a_frag[j] = A[m * 32 + k0 + j];       // A[m][k] row-major
    b_frag[j] = B[(k0 + j) * 16 + (lane & 15)];  // B[k][n] row-major
  }
  f32x4 acc = (f32x4)(0.0f);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_frag, b_frag, acc, 0, 0,
                                                0);
  int col = lane & 15;
  int row_base = (lane >> 4) * 4;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    D[(row_base + reg) * 16 + col] = acc[reg];
  }
}

void mfma_probe_launch(const void* A, const void* B, float* D,
                       hipStream_t stream) {
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, stream,
                     (const __bf16*)A, (const __bf16*)B, D);
}

// ---------------------------------------------------------------------
// fused forward for the same stem conv: out[K,32] = im2col(x)[K,256]
// @ W[256,32] + bias, x read directly as u8 (dequant fused).
// Per workgroup: 64 output rows x all 32 channels; K-loop over the 8
// patch rows (32 patch values each, one contiguous 32-byte u8
// segment per (k-row, patch-row) — same addressing as the wrw
// kernel). W (256x32 bf16, 16 KB) is staged to LDS once.
// ---------------------------------------------------------------------
#define FWD_ROWS 64  // k-rows (output pixels) per workgroup

__global__ __launch_bounds__(256)
void conv1_fwd_kernel(const unsigned char* __restrict__ frames,
                      const __bf16* __restrict__ weight,  // [256][32]
                      const float* __restrict__ bias,     // [32]
                      __bf16* __restrict__ out,           // [K][32]
                      int64_t K, float scale) {
  __shared__ __bf16 s_x[FWD_ROWS * 32];   // one patch-row chunk
  __shared__ __bf16 s_w[CONV1_N * 32];    // full weight, staged once

  const int tid = threadIdx.x;
  const int wave = tid / MA_WAVE;  // 0..3
  const int lane = tid % MA_WAVE;
  // wave -> (2 M-tiles of 16 rows) x (2 N-tiles of 16 cols): wave w
  // owns M-tile pair row (w&1) and N-tile (w>>1)
  const int wm = wave & 1;   // 0..1 -> rows wm*32 .. wm*32+31 (2 tiles)
  const int wn = wave >> 1;  // 0..1 -> cols wn*16 .. wn*16+15

  // stage the whole weight [256][32]
  for (int i = tid; i < CONV1_N * 32 / 8; i += 256) {
    ((bf16x8*)s_w)[i] = ((const bf16x8*)weight)[i];
  }

  const int64_t row0 = (int64_t)blockIdx.x * FWD_ROWS;
  f32x4 acc[2];  // two M-tiles (16x16 each) per wave
  acc[0] = (f32x4)(0.0f);
  acc[1] = (f32x4)(0.0f);
  __syncthreads();

  for (int pr = 0; pr < CONV1_KSZ; ++pr) {  // patch rows = K chunks
    // stage 64 k-rows x 32 patch values (u8 segment -> bf16)
    {
      int krow = tid >> 2;          // 0..63
      int quarter = tid & 3;        // 8 values each
      int64_t kk = row0 + krow;
      bf16x8 q;
#pragma unroll
      for (int j = 0; j < 8; ++j) q[j] = (__bf16)0.0f;
      if (kk < K) {
        int64_t b = kk / CONV1_POS;
        int pos = (int)(kk % CONV1_POS);
        int oh = pos / CONV1_OHW, ow = pos % CONV1_OHW;
        const unsigned char* src =
            frames
            + ((b * 84 + (int64_t)oh * CONV1_STRIDE + pr) * 84
               + (int64_t)ow * CONV1_STRIDE) * CONV1_CIN
            + quarter * 8;
        uint2 raw = *(const uint2*)src;
        unsigned int words[2] = {raw.x, raw.y};
#pragma unroll
        for (int w = 0; w < 2; ++w) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            q[w * 4 + j] = u8_bf16((words[w] >> (8 * j)) & 0xFF, scale);
          }
        }
      }
      *(bf16x8*)(s_x + krow * 32 + quarter * 8) = q;
    }
    __syncthreads();

    // MFMA over this chunk's K=32 (patch cols x channels)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      int m = wm * 32 + mt * 16 + (lane & 15);
      int k0 = (lane >> 4) * 8;
      // A[m][k]: contiguous along k -> one vector read
      bf16x8 a_frag = *(bf16x8*)(s_x + m * 32 + k0);
      bf16x8 b_frag;
      int n = wn * 16 + (lane & 15);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        b_frag[j] = s_w[(pr * 32 + k0 + j) * 32 + n];
      }
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_frag, b_frag, acc[mt], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue: bias add, bf16 store (C/D map: col=lane&15,
  // row=(lane>>4)*4+reg)
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    int col = wn * 16 + (lane & 15);
    float b = bias != nullptr ? bias[col] : 0.0f;
    int row_base = wm * 32 + mt * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int64_t kk = row0 + row_base + reg;
      if (kk < K) {
        out[kk * 32 + col] = (__bf16)(acc[mt][reg] + b);
      }
    }
  }
}

void conv1_fwd_launch(const unsigned char* frames, const void* weight,
                      const float* bias, void* out, int64_t K,
                      float scale, hipStream_t stream) {
  int64_t grid = (K + FWD_ROWS - 1) / FWD_ROWS;
  const char* ver = getenv("MACHIN_CONV1_V");
  int v = ver ? atoi(ver) : 4;
  if (v != 1 && v != 2 && v != 3 &&
      conv1_fwd_v4_launch(frames, weight, bias, out, nullptr, false, K,
                          scale, stream)) {
    return;
  }
  if (v == 1) {
    hipLaunchKernelGGL(conv1_fwd_kernel, dim3((unsigned)grid), dim3(256),
                       0, stream, frames, (const __bf16*)weight, bias,
                       (__bf16*)out, K, scale);
  } else if (v == 2) {
    hipLaunchKernelGGL(conv1_fwd_v2_kernel, dim3((unsigned)grid),
                       dim3(256), 0, stream, frames,
                       (const __bf16*)weight, bias, (__bf16*)out, K,
                       scale);
  } else {
    int64_t grid3 = (K + 127) / 128;  // FWD3_ROWS
    hipLaunchKernelGGL(conv1_fwd_v3_kernel, dim3((unsigned)grid3),
                       dim3(256), 0, stream, frames,
                       (const __bf16*)weight, bias, (__bf16*)out, K,
                       scale);
  }
  HIP_CHECK(hipGetLastError());
}

// =====================================================================
// v2 kernels: tiled LDS images + ds_read_b64_tr_b16 fragment loads.
//
// v1 profile (round-1 VERDICT weak #6): the MFMA operand loads were
// per-element ds_read_u16 (72 narrow reads per wave per K-chunk) —
// LDS-instruction-bound at 1.80 ms wrw / 1.46 ms fwd vs a ~0.4 ms
// HBM bound.
//
// ds_read_b64_tr_b16 semantics, pinned by tools/probe_tr16.py on
// hardware (gpurun_out/tr16_probe2.log): lanes operate in clusters
// of 4; the cluster reads one CONTIGUOUS 32 B window (a 4x4 bf16
// tile, row-major [row][col]) at the cluster's (shared) address, and
// lane l receives COLUMN (l&3): elements win[(l&3) + j*4], j=0..3.
// Address bits 3-4 are ignored (windows must be 32 B aligned); the
// offset immediate is additive in the same masked address space.
//
// So the LDS images are [n_cluster][k_quad][4][4] bf16 tilings: one
// 16x16x32 MFMA B-fragment = TWO tr reads (k 8-rows = two stacked
// 4x4 windows, second via offset:32). Per wave per chunk: 18 LDS
// reads vs v1's 72.
//
// x image: [nc 64][kq 8][4][4]  elem (k, c):
//   addr = (c>>2)*128 + (k>>2)*16 + (k&3)*4 + (c&3)
// dy image: [nc 8][kq 8][4][4] with the same windows.
//
// RETIRED, and corrected: the semantics above are incomplete. The later
// probes (see the v3 header) showed that the 16 lanes of a quarter
// receive only 16 distinct values, rows of the four subgroup leaders'
// windows, so the read cannot deliver a 16x16x32 fragment. The exact
// tests (tests/test_stem_conv_gpu.py) showed what that meant for these
// kernels: every forward output and every weight-gradient element was
// wrong, and the bias gradient held 4 distinct values per 16 channels
// (channel c got the sum of channel c & 3 of its tile). The fragments
// are now gathered from the same tiled images with plain LDS reads
// (tile_frag below), which makes v2 correct and no faster than v1; the
// transpose reads remain in the probes only.
// =====================================================================
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// NOTE the explicit s_waitcnt: the compiler does not track inline-asm
// DS reads, so without it the destination registers are consumed
// before the LDS data lands (first probe run returned garbage).
__device__ __forceinline__ bf16x4 ds_tr16(const __bf16* addr) {
  bf16x4 out;
  asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(out)
               : "v"((unsigned)(uintptr_t)addr)
               : "memory");
  return out;
}

__device__ __forceinline__ bf16x4 ds_tr16_off128(const __bf16* addr) {
  bf16x4 out;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %1 offset:32\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(out)
      : "v"((unsigned)(uintptr_t)addr)
      : "memory");
  return out;
}

// fused pair: both k-tiles of one fragment, ONE waitcnt
__device__ __forceinline__ void ds_tr16_pair(const __bf16* addr,
                                             bf16x4& lo, bf16x4& hi) {
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %2 offset:32\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(lo), "=&v"(hi)
      : "v"((unsigned)(uintptr_t)addr)
      : "memory");
}

__device__ __forceinline__ bf16x4 lo4(bf16x8 v) {
  bf16x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = v[j];
  return r;
}

__device__ __forceinline__ bf16x4 hi4(bf16x8 v) {
  bf16x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = v[4 + j];
  return r;
}

__device__ __forceinline__ void pack8(bf16x8& dst, bf16x4 lo, bf16x4 hi) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    dst[j] = lo[j];
    dst[4 + j] = hi[j];
  }
}

// One lane's MFMA fragment from a [nc][kq][4][4] tiled image: `base`
// points at k-quad 2g of the lane's n-cluster (g = lane >> 4); element j
// is row k = 8g + j, column lane & 3 of the cluster, i.e. row j & 3 of
// window j >> 2.
__device__ __forceinline__ bf16x8 tile_frag(const __bf16* base, int lane) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = base[(j >> 2) * 16 + (j & 3) * 4 + (lane & 3)];
  }
  return v;
}

__global__ __launch_bounds__(256)
void conv1_wrw_v2_kernel(const __bf16* __restrict__ dy,
                         const unsigned char* __restrict__ frames,
                         float* __restrict__ out,
                         float* __restrict__ b_out, int64_t K,
                         int64_t k_per_wg, float scale) {
  __shared__ __bf16 s_dy[2 * 8 * 64];   // [mt][kt][4][16]
  __shared__ __bf16 s_x[16 * 8 * 64];   // [nt][kt][4][16]

  const int tid = threadIdx.x;
  const int wave = tid / MA_WAVE;
  const int lane = tid % MA_WAVE;
  const int mt = wave & 1;
  const int ng = wave >> 1;

  f32x4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = (f32x4)(0.0f);
  float bias_acc = 0.0f;

  // per-lane window base addresses (constant across the K loop):
  // cluster (lane&15)>>2 picks the n-quad; k-group g = lane>>4 needs
  // k-quads 2g (base) and 2g+1 (offset:32)
  const __bf16* a_base = s_dy + (mt * 4 + ((lane & 15) >> 2)) * 128
                         + (lane >> 4) * 32;
  const __bf16* b_base = s_x + (ng * 32 + ((lane & 15) >> 2)) * 128
                         + (lane >> 4) * 32;

  const int64_t k_begin = (int64_t)blockIdx.x * k_per_wg;
  const int64_t k_end = min(k_begin + k_per_wg, K);

  for (int64_t kc = k_begin; kc < k_end; kc += KC) {
    // ---- stage dy chunk into [mt][kt][4][16] tiles ----------------
    if (tid < 128) {
      int row = tid >> 2;        // k-row 0..31
      int seg = tid & 3;         // 8 cols each
      int64_t kk = kc + row;
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.0f;
      float bsum = 0.0f;
      if (kk < k_end) {
        v = *(const bf16x8*)(dy + kk * CONV1_COUT + seg * 8);
      }
      // cols seg*8..seg*8+7 span n-clusters 2*seg and 2*seg+1
      __bf16* base = s_dy + (row >> 2) * 16 + (row & 3) * 4;
      *(bf16x4*)(base + (seg * 2) * 128) =
          lo4(v);
      *(bf16x4*)(base + (seg * 2 + 1) * 128) =
          hi4(v);
      (void)bsum;
    }
    // ---- stage x chunk into [nt][kt][4][16] tiles -----------------
    // thread (krow = tid&31, r = tid>>3? ) -> mapping: krow low bits
    // keeps the 8-lane write groups on distinct banks
    {
      int krow = tid & 31;
      int r = tid >> 5;          // patch row 0..7
      int64_t kk = kc + krow;
      bf16x8 q0, q1, q2, q3;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        q0[j] = (__bf16)0.0f;
        q1[j] = (__bf16)0.0f;
        q2[j] = (__bf16)0.0f;
        q3[j] = (__bf16)0.0f;
      }
      if (kk < k_end) {
        int64_t b = kk / CONV1_POS;
        int pos = (int)(kk % CONV1_POS);
        int oh = pos / CONV1_OHW, ow = pos % CONV1_OHW;
        const unsigned char* src =
            frames
            + ((b * 84 + (int64_t)oh * CONV1_STRIDE + r) * 84
               + (int64_t)ow * CONV1_STRIDE) * CONV1_CIN;
        uint4 raw0 = *(const uint4*)src;
        uint4 raw1 = *(const uint4*)(src + 16);
        unsigned int words[8] = {raw0.x, raw0.y, raw0.z, raw0.w,
                                 raw1.x, raw1.y, raw1.z, raw1.w};
#pragma unroll
        for (int w = 0; w < 2; ++w) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            q0[w * 4 + j] = u8_bf16((words[w] >> (8 * j)) & 0xFF, scale);
            q1[w * 4 + j] =
                u8_bf16((words[w + 2] >> (8 * j)) & 0xFF, scale);
            q2[w * 4 + j] =
                u8_bf16((words[w + 4] >> (8 * j)) & 0xFF, scale);
            q3[w * 4 + j] =
                u8_bf16((words[w + 6] >> (8 * j)) & 0xFF, scale);
          }
        }
      }
      // cols r*32 .. r*32+31 span n-clusters r*8 .. r*8+7; each
      // 4-col piece is one contiguous window row (8 B write)
      __bf16* base = s_x + (krow >> 2) * 16 + (krow & 3) * 4
                     + (r * 8) * 128;
      *(bf16x4*)(base + 0 * 128) = lo4(q0);
      *(bf16x4*)(base + 1 * 128) = hi4(q0);
      *(bf16x4*)(base + 2 * 128) = lo4(q1);
      *(bf16x4*)(base + 3 * 128) = hi4(q1);
      *(bf16x4*)(base + 4 * 128) = lo4(q2);
      *(bf16x4*)(base + 5 * 128) = hi4(q2);
      *(bf16x4*)(base + 6 * 128) = lo4(q3);
      *(bf16x4*)(base + 7 * 128) = hi4(q3);
    }
    __syncthreads();

    // ---- fragments from the tiled images -------------------------
    bf16x8 a_frag = tile_frag(a_base, lane);
    // fused bias from the fragment already in registers: lane group g
    // of an ng==0 wave holds dy[k=8g..8g+7][col mt*16+(lane&15)]
    if (ng == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) bias_acc += (float)a_frag[j];
    }
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      bf16x8 b_frag = tile_frag(b_base + nt * 512, lane);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_frag, b_frag, acc[nt], 0, 0, 0);
    }
    __syncthreads();
  }

  if (ng == 0) {
    // reduce the 4 lane groups' partial column sums, then one
    // atomic per column from lanes 0..15
    bias_acc += __shfl_down(bias_acc, 32, 64);
    bias_acc += __shfl_down(bias_acc, 16, 64);
    if (lane < 16) atomicAdd(&b_out[mt * 16 + lane], bias_acc);
  }
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) {
    int col = (ng * 8 + nt) * 16 + (lane & 15);
    int row_base = mt * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      atomicAdd(&out[(row_base + reg) * CONV1_N + col], acc[nt][reg]);
    }
  }
}

// fwd v2: weight staged ONCE into [nc 8][kq 64][4][4] windows; the
// B fragment is gathered once per (pr) chunk, hoisted out of the mt
// loop (v1 re-read it per m-tile).
__global__ __launch_bounds__(256)
void conv1_fwd_v2_kernel(const unsigned char* __restrict__ frames,
                         const __bf16* __restrict__ weight,  // [256][32]
                         const float* __restrict__ bias,
                         __bf16* __restrict__ out, int64_t K,
                         float scale) {
  __shared__ __bf16 s_x[FWD_ROWS * 32];
  __shared__ __bf16 s_w[2 * 64 * 64];  // [nt][kt][4][16]

  const int tid = threadIdx.x;
  const int wave = tid / MA_WAVE;
  const int lane = tid % MA_WAVE;
  const int wm = wave & 1;
  const int wn = wave >> 1;

  // stage weight into [nc 8][kq 64][4][4] windows: thread tid owns
  // row k=tid (32 cols -> 8 clusters, one 8 B write each)
  {
    int k = tid;
    bf16x8 r0 = ((const bf16x8*)(weight + k * 32))[0];
    bf16x8 r1 = ((const bf16x8*)(weight + k * 32))[1];
    bf16x8 r2 = ((const bf16x8*)(weight + k * 32))[2];
    bf16x8 r3 = ((const bf16x8*)(weight + k * 32))[3];
    __bf16* base = s_w + (k >> 2) * 16 + (k & 3) * 4;
    *(bf16x4*)(base + 0 * 1024) = lo4(r0);
    *(bf16x4*)(base + 1 * 1024) = hi4(r0);
    *(bf16x4*)(base + 2 * 1024) = lo4(r1);
    *(bf16x4*)(base + 3 * 1024) = hi4(r1);
    *(bf16x4*)(base + 4 * 1024) = lo4(r2);
    *(bf16x4*)(base + 5 * 1024) = hi4(r2);
    *(bf16x4*)(base + 6 * 1024) = lo4(r3);
    *(bf16x4*)(base + 7 * 1024) = hi4(r3);
  }

  const int64_t row0 = (int64_t)blockIdx.x * FWD_ROWS;
  f32x4 acc[2];
  acc[0] = (f32x4)(0.0f);
  acc[1] = (f32x4)(0.0f);
  const __bf16* w_base = s_w + (wn * 4 + ((lane & 15) >> 2)) * 1024
                         + (lane >> 4) * 32;
  __syncthreads();

  for (int pr = 0; pr < CONV1_KSZ; ++pr) {
    {
      int krow = tid >> 2;
      int quarter = tid & 3;
      int64_t kk = row0 + krow;
      bf16x8 q;
#pragma unroll
      for (int j = 0; j < 8; ++j) q[j] = (__bf16)0.0f;
      if (kk < K) {
        int64_t b = kk / CONV1_POS;
        int pos = (int)(kk % CONV1_POS);
        int oh = pos / CONV1_OHW, ow = pos % CONV1_OHW;
        const unsigned char* src =
            frames
            + ((b * 84 + (int64_t)oh * CONV1_STRIDE + pr) * 84
               + (int64_t)ow * CONV1_STRIDE) * CONV1_CIN
            + quarter * 8;
        uint2 raw = *(const uint2*)src;
        unsigned int words[2] = {raw.x, raw.y};
#pragma unroll
        for (int w = 0; w < 2; ++w) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            q[w * 4 + j] = u8_bf16((words[w] >> (8 * j)) & 0xFF, scale);
          }
        }
      }
      *(bf16x8*)(s_x + krow * 32 + quarter * 8) = q;
    }
    __syncthreads();

    // B fragment for this pr chunk: k-quads pr*8 + {2g, 2g+1}
    bf16x8 b_frag = tile_frag(w_base + pr * 8 * 16, lane);
#pragma unroll
    for (int mt2 = 0; mt2 < 2; ++mt2) {
      int m = wm * 32 + mt2 * 16 + (lane & 15);
      int k0 = (lane >> 4) * 8;
      bf16x8 a_frag = *(bf16x8*)(s_x + m * 32 + k0);
      acc[mt2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_frag, b_frag, acc[mt2], 0, 0, 0);
    }
    __syncthreads();
  }

#pragma unroll
  for (int mt2 = 0; mt2 < 2; ++mt2) {
    int col = wn * 16 + (lane & 15);
    float b = bias != nullptr ? bias[col] : 0.0f;
    int row_base = wm * 32 + mt2 * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      int64_t kk = row0 + row_base + reg;
      if (kk < K) {
        out[kk * 32 + col] = (__bf16)(acc[mt2][reg] + b);
      }
    }
  }
}

// ---------------------------------------------------------------------
// tr16 probe: pins the exact ds_read_b64_tr_b16 lane/element mapping
// on hardware before the conv kernels trust it (same methodology as
// mfma_probe). LDS is filled with lds[i] = i; each lane issues the
// read with a configurable per-lane address and reports its 4
// elements. mode 0: uniform tile base. mode 1: base + (lane&15)*2 B.
// mode 2: base + lane*2 B. mode 3: base + (lane>>4)*128 B.
// ---------------------------------------------------------------------
__global__ void tr16_probe_kernel(float* __restrict__ out, int mode) {
  __shared__ __bf16 l[1024];
  for (int i = threadIdx.x; i < 1024; i += blockDim.x) {
    l[i] = (__bf16)(float)i;
  }
  __syncthreads();
  int lane = threadIdx.x;
  const __bf16* addr = l;
  if (mode == 1) addr += (lane & 15);
  if (mode == 2) addr += lane;
  if (mode == 3) addr += (lane >> 4) * 64;
  if (mode == 4) addr += (lane & 15) + (lane >> 4) * 64;
  bf16x4 v = ds_tr16(addr);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    out[lane * 4 + j] = (float)v[j];
  }
}

void tr16_probe_launch(float* out, int mode, hipStream_t stream) {
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 0, stream,
                     out, mode);
  HIP_CHECK(hipGetLastError());
}

// fwd B-fragment probe: stages a synthetic weight through the EXACT
// v2 staging code, reads fragments with the EXACT v2 addressing, and
// dumps every lane's 8 elements. which=0: W[k][n]=k (checks the k
// mapping); which=1: W[k][n]=n (checks the n mapping).
// out: [2 pr][256 threads][8]
__global__ __launch_bounds__(256)
void fwd_bfrag_probe_kernel(float* __restrict__ out, int which) {
  __shared__ __bf16 s_w[2 * 64 * 64];
  const int tid = threadIdx.x;
  const int wave = tid / MA_WAVE;
  const int lane = tid % MA_WAVE;
  const int wn = wave >> 1;

  {
    int k = tid;
    bf16x8 r0, r1, r2, r3;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      r0[j] = (__bf16)(float)(which == 0 ? k : j);
      r1[j] = (__bf16)(float)(which == 0 ? k : 8 + j);
      r2[j] = (__bf16)(float)(which == 0 ? k : 16 + j);
      r3[j] = (__bf16)(float)(which == 0 ? k : 24 + j);
    }
    __bf16* base = s_w + (k >> 2) * 16 + (k & 3) * 4;
    *(bf16x4*)(base + 0 * 1024) = lo4(r0);
    *(bf16x4*)(base + 1 * 1024) = hi4(r0);
    *(bf16x4*)(base + 2 * 1024) = lo4(r1);
    *(bf16x4*)(base + 3 * 1024) = hi4(r1);
    *(bf16x4*)(base + 4 * 1024) = lo4(r2);
    *(bf16x4*)(base + 5 * 1024) = hi4(r2);
    *(bf16x4*)(base + 6 * 1024) = lo4(r3);
    *(bf16x4*)(base + 7 * 1024) = hi4(r3);
  }
  const __bf16* w_base = s_w + (wn * 4 + ((lane & 15) >> 2)) * 1024
                         + (lane >> 4) * 32;
  __syncthreads();
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    const __bf16* wb = w_base + pr * 8 * 16;
    bf16x4 lo, hi;
    ds_tr16_pair(wb, lo, hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out[(pr * 256 + tid) * 8 + j] = (float)lo[j];
      out[(pr * 256 + tid) * 8 + 4 + j] = (float)hi[j];
    }
  }
}

void fwd_bfrag_probe_launch(float* out, int which, hipStream_t stream) {
  hipLaunchKernelGGL(fwd_bfrag_probe_kernel, dim3(1), dim3(256), 0,
                     stream, out, which);
  HIP_CHECK(hipGetLastError());
}

// Decisive tr16 diagnostics.
// mode 0/1: stage synthetic W (value = k for 0, n for 1) through the
//   v2 staging code, then dump the raw LDS image LINEARLY (plain
//   reads — isolates staging correctness from the tr16 read).
// mode 2/3: fill s_w[i] = i&255 (2) or i>>8 (3) DIRECTLY, then tr16-
//   read with the exact fwd fragment addressing and dump per-lane
//   elements (isolates the read's element map; combining both runs
//   reconstructs exact LDS indices).
// out: 8192 floats for modes 0/1; [2][256][8] for modes 2/3.
__global__ __launch_bounds__(256)
void tr16_diag_kernel(float* __restrict__ out, int mode) {
  __shared__ __bf16 s_w[2 * 64 * 64];
  const int tid = threadIdx.x;
  const int wave = tid / MA_WAVE;
  const int lane = tid % MA_WAVE;
  const int wn = wave >> 1;

  if (mode <= 1) {
    int k = tid;
    bf16x8 r0, r1, r2, r3;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      r0[j] = (__bf16)(float)(mode == 0 ? k : j);
      r1[j] = (__bf16)(float)(mode == 0 ? k : 8 + j);
      r2[j] = (__bf16)(float)(mode == 0 ? k : 16 + j);
      r3[j] = (__bf16)(float)(mode == 0 ? k : 24 + j);
    }
    __bf16* base = s_w + (k >> 2) * 16 + (k & 3) * 4;
    *(bf16x4*)(base + 0 * 1024) = lo4(r0);
    *(bf16x4*)(base + 1 * 1024) = hi4(r0);
    *(bf16x4*)(base + 2 * 1024) = lo4(r1);
    *(bf16x4*)(base + 3 * 1024) = hi4(r1);
    *(bf16x4*)(base + 4 * 1024) = lo4(r2);
    *(bf16x4*)(base + 5 * 1024) = hi4(r2);
    *(bf16x4*)(base + 6 * 1024) = lo4(r3);
    *(bf16x4*)(base + 7 * 1024) = hi4(r3);
    __syncthreads();
    for (int i = tid; i < 8192; i += 256) {
      out[i] = (float)s_w[i];
    }
    return;
  }

  for (int i = tid; i < 8192; i += 256) {
    s_w[i] = (__bf16)(float)(mode == 2 ? (i & 255) : (i >> 8));
  }
  __syncthreads();
  const __bf16* w_base = s_w + (wn * 4 + ((lane & 15) >> 2)) * 1024
                         + (lane >> 4) * 32;
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    const __bf16* wb = w_base + pr * 8 * 16;
    bf16x4 lo, hi;
    ds_tr16_pair(wb, lo, hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      out[(pr * 256 + tid) * 8 + j] = (float)lo[j];
      out[(pr * 256 + tid) * 8 + 4 + j] = (float)hi[j];
    }
  }
}

void tr16_diag_launch(float* out, int mode, hipStream_t stream) {
  hipLaunchKernelGGL(tr16_diag_kernel, dim3(1), dim3(256), 0, stream,
                     out, mode);
  HIP_CHECK(hipGetLastError());
}

// =====================================================================
// v3 kernels: per-lane FRAGMENT-ORDER LDS images (guide §7: fix
// ds_read_u16 with a contiguous fragment layout).
//
// The tr16 probes (tools/probe_tr16_diag.py) showed the transpose-
// read delivers only 16 distinct values per 16-lane quarter (rows
// from the four subgroup-leader addresses, column l&3), so it cannot
// feed full 16x16x32 fragments any cheaper than scalar reads. v3
// instead stores each lane's fragment elements CONTIGUOUSLY: the
// staging threads load k-strided global words and transpose u8/bf16
// blocks in registers, so every MFMA operand becomes ONE
// ds_read_b128 per k-step. Per wave per 64-k chunk: 18 wide reads +
// 16 MFMAs (v1: 144 scalar reads + 16 MFMAs).
//
// x image (per n-tile nt): slot(l) = (l>>3)*136 + (l&7)*16 elems
// (16 B pad per 8 lanes keeps the b128 lane banks distinct);
// slot holds [s in 2][8] = x[k = s*32 + (l>>4)*8 + j][nt*16+(l&15)].
// =====================================================================
#define KC3 64
#define DY3_MT 1088   // per-m-tile image elems: 8 groups x 136
#define X3_NT 1088    // per-n-tile image elems

__device__ __forceinline__ int frag_slot(int lane) {
  return (lane >> 3) * 136 + (lane & 7) * 16;
}

// MASKED: the ReLU of the stem is fused into this kernel's dy load.
// mask[k] holds the sign pattern of output row k (bit c set <=> the
// activated output y[k][c] > 0, written by the fused forward); dy
// elements whose bit is clear are zeroed before the fragment image is
// written, so both the MFMA operand and the bias sum see
// relu'(y) * dy and the 1 GB threshold_backward pass disappears.
template <bool MASKED>
__device__ __forceinline__
void conv1_wrw_v3_body(const __bf16* __restrict__ dy,
                       const unsigned int* __restrict__ mask,
                       const unsigned char* __restrict__ frames,
                       float* __restrict__ out,
                       float* __restrict__ b_out, int64_t K,
                       int64_t k_per_wg, float scale) {
  __shared__ __bf16 s_dy[2 * DY3_MT];
  __shared__ __bf16 s_x[16 * X3_NT];

  const int tid = threadIdx.x;
  const int wave = tid / MA_WAVE;
  const int lane = tid % MA_WAVE;
  const int mt = wave & 1;
  const int ng = wave >> 1;

  f32x4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = (f32x4)(0.0f);
  float bias_acc = 0.0f;

  const __bf16* a_base = s_dy + mt * DY3_MT + frag_slot(lane);
  const __bf16* b_base = s_x + ng * 8 * X3_NT + frag_slot(lane);

  const int64_t k_begin = (int64_t)blockIdx.x * k_per_wg;
  const int64_t k_end = min(k_begin + k_per_wg, K);

  // register prefetch: global loads for chunk kc+KC3 are issued while
  // the MFMAs for chunk kc run (PMC showed 35-48% SQ_WAIT_ANY =
  // waves parked on global latency with a serial stage->barrier->
  // MFMA loop)
  const int x_ngc = tid & 63, x_kg = tid >> 6;  // x block 1 of 2
  const int x_ngc2 = x_ngc, x_kg2 = x_kg + 4;   // x block 2
  const int dy_mg = tid & 7, dy_kg = tid >> 3;  // dy block (tid<64)

  auto load_x = [&](int64_t kc, int ngc, int kg, unsigned int* d) {
    int r = ngc >> 3;
    int dword_off = (ngc & 7) * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int64_t kk = kc + kg * 8 + i;
      d[i] = 0u;
      if (kk < k_end) {
        int64_t b = kk / CONV1_POS;
        int pos = (int)(kk % CONV1_POS);
        int oh = pos / CONV1_OHW, ow = pos % CONV1_OHW;
        d[i] = *(const unsigned int*)(
            frames
            + ((b * 84 + (int64_t)oh * CONV1_STRIDE + r) * 84
               + (int64_t)ow * CONV1_STRIDE) * CONV1_CIN
            + dword_off);
      }
    }
  };
  // the mask words ride along with the prefetched dy rows and are
  // applied when the chunk is written to LDS, so the loads still
  // complete under the previous chunk's MFMAs
  auto load_dy = [&](int64_t kc, bf16x4* ld, unsigned int* mw) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int64_t kk = kc + dy_kg * 8 + i;
      if (kk < k_end) {
        ld[i] = *(const bf16x4*)(dy + kk * CONV1_COUT + dy_mg * 4);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) ld[i][j] = (__bf16)0.0f;
      }
    }
    if constexpr (MASKED) {
      // the 8 rows of this lane start at a multiple of 8 (k_begin is a
      // multiple of KC3) and K = batch*400 is one too, so the 8 words
      // are 32 B aligned and all inside or all outside [0, k_end):
      // two 16 B loads instead of eight 4 B ones
      int64_t k0 = kc + dy_kg * 8;
      uint4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
      if (k0 < k_end) {
        lo = *(const uint4*)(mask + k0);
        hi = *(const uint4*)(mask + k0 + 4);
      }
      mw[0] = lo.x; mw[1] = lo.y; mw[2] = lo.z; mw[3] = lo.w;
      mw[4] = hi.x; mw[5] = hi.y; mw[6] = hi.z; mw[7] = hi.w;
    }
  };
  auto store_x = [&](int ngc, int kg, const unsigned int* d) {
    int s = kg >> 2, q = kg & 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int n = ngc * 4 + j;
      int l = q * 16 + (n & 15);
      bf16x8 v;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        v[i] = u8_bf16((d[i] >> (8 * j)) & 0xFF, scale);
      }
      *(bf16x8*)(s_x + (n >> 4) * X3_NT + frag_slot(l) + s * 8) = v;
    }
  };

  unsigned int d1[8], d2[8];
  bf16x4 ldy[8];
  unsigned int mw[8];
  load_x(k_begin, x_ngc, x_kg, d1);
  load_x(k_begin, x_ngc2, x_kg2, d2);
  if (tid < 64) load_dy(k_begin, ldy, mw);

  for (int64_t kc = k_begin; kc < k_end; kc += KC3) {
    // write the prefetched chunk into the fragment images
    if (tid < 64) {
      int s = dy_kg >> 2, q = dy_kg & 3;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int m = dy_mg * 4 + j;
        int l = q * 16 + (m & 15);
        bf16x8 v;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if constexpr (MASKED) {
            v[i] = ((mw[i] >> m) & 1u) ? ldy[i][j] : (__bf16)0.0f;
          } else {
            v[i] = ldy[i][j];
          }
        }
        *(bf16x8*)(s_dy + (m >> 4) * DY3_MT + frag_slot(l)
                   + s * 8) = v;
      }
    }
    store_x(x_ngc, x_kg, d1);
    store_x(x_ngc2, x_kg2, d2);
    __syncthreads();

    // issue next chunk's global loads, then MFMA over this chunk —
    // the loads complete under the MFMAs
    if (kc + KC3 < k_end) {
      load_x(kc + KC3, x_ngc, x_kg, d1);
      load_x(kc + KC3, x_ngc2, x_kg2, d2);
      if (tid < 64) load_dy(kc + KC3, ldy, mw);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 a_frag = *(const bf16x8*)(a_base + s * 8);
      if (ng == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bias_acc += (float)a_frag[j];
      }
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        bf16x8 b_frag = *(const bf16x8*)(b_base + nt * X3_NT + s * 8);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag, b_frag, acc[nt], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  if (ng == 0) {
    bias_acc += __shfl_down(bias_acc, 32, 64);
    bias_acc += __shfl_down(bias_acc, 16, 64);
    if (lane < 16) atomicAdd(&b_out[mt * 16 + lane], bias_acc);
  }
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) {
    int col = (ng * 8 + nt) * 16 + (lane & 15);
    int row_base = mt * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      atomicAdd(&out[(row_base + reg) * CONV1_N + col], acc[nt][reg]);
    }
  }
}

__global__ __launch_bounds__(256)
void conv1_wrw_v3_kernel(const __bf16* __restrict__ dy,
                         const unsigned char* __restrict__ frames,
                         float* __restrict__ out,
                         float* __restrict__ b_out, int64_t K,
                         int64_t k_per_wg, float scale) {
  conv1_wrw_v3_body<false>(dy, nullptr, frames, out, b_out, K, k_per_wg,
                           scale);
}

__global__ __launch_bounds__(256)
void conv1_wrw_v3_masked_kernel(const __bf16* __restrict__ dy,
                                const unsigned int* __restrict__ mask,
                                const unsigned char* __restrict__ frames,
                                float* __restrict__ out,
                                float* __restrict__ b_out, int64_t K,
                                int64_t k_per_wg, float scale) {
  conv1_wrw_v3_body<true>(dy, mask, frames, out, b_out, K, k_per_wg,
                          scale);
}

// fwd v3: 128 output rows per workgroup (16 MFMAs between barrier
// pairs instead of 8) with register-prefetched frame loads — the PMC
// run showed fwd 71% SQ_WAIT_ANY (waves parked on global latency in
// a serial stage->barrier->MFMA loop). Weight staged ONCE into a
// fragment-order image; per pr-chunk each B fragment is one
// ds_read_b128 shared across both m-tiles of the wave.
// w image: addr(wn, l, pr) = wn*4624 + (l>>4)*1156 + (l&15)*72
//          + pr*8   (4-elem pad per quarter, 8 per lane slot)
//
// RELU: the epilogue stores relu(bf16(acc + bias)) — the same bits as
// relu applied to the plain kernel's output — and writes the sign
// pattern of every output row as one 32-bit word (bit c set <=>
// channel c > 0) for the masked weight-gradient kernel.
// The stores stay sixteen 2-byte stores per lane: staging the tile
// through s_x to leave as 16 B per lane was traced slower (1.49 vs
// 1.39 ms at batch 40960, profiles/); it adds a barrier and an LDS
// round trip, and the cause was not looked into further.
#define FWD3_ROWS 128

template <bool RELU>
__device__ __forceinline__
void conv1_fwd_v3_body(const unsigned char* __restrict__ frames,
                       const __bf16* __restrict__ weight,  // [256][32]
                       const float* __restrict__ bias,
                       __bf16* __restrict__ out,
                       unsigned int* __restrict__ mask, int64_t K,
                       float scale) {
  __shared__ __bf16 s_x[FWD3_ROWS * 32];
  __shared__ __bf16 s_w[2 * 4624];

  const int tid = threadIdx.x;
  const int wave = tid / MA_WAVE;  // wave w owns rows w*32..w*32+31
  const int lane = tid % MA_WAVE;

  {
    int k = tid;  // one weight row per thread
    int pr = k >> 5, q = (k >> 3) & 3, i = k & 7;
    bf16x8 r0 = ((const bf16x8*)(weight + k * 32))[0];
    bf16x8 r1 = ((const bf16x8*)(weight + k * 32))[1];
    bf16x8 r2 = ((const bf16x8*)(weight + k * 32))[2];
    bf16x8 r3 = ((const bf16x8*)(weight + k * 32))[3];
#pragma unroll
    for (int n16 = 0; n16 < 16; ++n16) {
      int l = q * 16 + n16;
      s_w[(l >> 4) * 1156 + (l & 15) * 72 + pr * 8 + i] =
          n16 < 8 ? r0[n16] : r1[n16 - 8];
      s_w[4624 + (l >> 4) * 1156 + (l & 15) * 72 + pr * 8 + i] =
          n16 < 8 ? r2[n16] : r3[n16 - 8];
    }
  }

  const int64_t row0 = (int64_t)blockIdx.x * FWD3_ROWS;
  f32x4 acc[2][2];  // [m-tile][n-tile]
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    acc[a][0] = (f32x4)(0.0f);
    acc[a][1] = (f32x4)(0.0f);
  }
  const __bf16* w_base = s_w + (lane >> 4) * 1156 + (lane & 15) * 72;

  // staging: 2 threads per row, 16 B each
  const int st_row = tid >> 1, st_half = tid & 1;
  const int64_t st_kk = row0 + st_row;
  const unsigned char* st_src = nullptr;
  if (st_kk < K) {
    int64_t b = st_kk / CONV1_POS;
    int pos = (int)(st_kk % CONV1_POS);
    int oh = pos / CONV1_OHW, ow = pos % CONV1_OHW;
    st_src = frames
             + ((b * 84 + (int64_t)oh * CONV1_STRIDE) * 84
                + (int64_t)ow * CONV1_STRIDE) * CONV1_CIN
             + st_half * 16;
  }

  uint4 raw = {0u, 0u, 0u, 0u};
  if (st_src != nullptr) raw = *(const uint4*)st_src;  // pr=0
  __syncthreads();  // weight image ready

  for (int pr = 0; pr < CONV1_KSZ; ++pr) {
    {
      unsigned int words[4] = {raw.x, raw.y, raw.z, raw.w};
      bf16x8 q0, q1;
#pragma unroll
      for (int w = 0; w < 2; ++w) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          q0[w * 4 + j] = u8_bf16((words[w] >> (8 * j)) & 0xFF, scale);
          q1[w * 4 + j] =
              u8_bf16((words[w + 2] >> (8 * j)) & 0xFF, scale);
        }
      }
      *(bf16x8*)(s_x + st_row * 32 + st_half * 16) = q0;
      *(bf16x8*)(s_x + st_row * 32 + st_half * 16 + 8) = q1;
    }
    __syncthreads();
    // prefetch next patch row while the MFMAs below run
    if (pr + 1 < CONV1_KSZ && st_src != nullptr) {
      raw = *(const uint4*)(st_src + (int64_t)(pr + 1) * 84
                            * CONV1_CIN);
    }
    bf16x8 b0 = *(const bf16x8*)(w_base + pr * 8);
    bf16x8 b1 = *(const bf16x8*)(w_base + 4624 + pr * 8);
#pragma unroll
    for (int mt2 = 0; mt2 < 2; ++mt2) {
      int m = wave * 32 + mt2 * 16 + (lane & 15);
      int k0 = (lane >> 4) * 8;
      bf16x8 a_frag = *(bf16x8*)(s_x + m * 32 + k0);
      acc[mt2][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_frag, b0, acc[mt2][0], 0, 0, 0);
      acc[mt2][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_frag, b1, acc[mt2][1], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue (C/D map: col=lane&15, row=(lane>>4)*4+reg)
  const int col0 = lane & 15;
  const float bias0 = bias != nullptr ? bias[col0] : 0.0f;
  const float bias1 = bias != nullptr ? bias[16 + col0] : 0.0f;
  unsigned int row_mask = 0u;  // lanes 0..31: word of row wave*32+lane
#pragma unroll
  for (int mt2 = 0; mt2 < 2; ++mt2) {
    int row_base = wave * 32 + mt2 * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      __bf16 v0 = (__bf16)(acc[mt2][0][reg] + bias0);
      __bf16 v1 = (__bf16)(acc[mt2][1][reg] + bias1);
      if constexpr (RELU) {
        // !(v <= 0) keeps NaN, as ATen's relu does
        bool p0 = !((float)v0 <= 0.0f);
        bool p1 = !((float)v1 <= 0.0f);
        // ballot bit l = lane l = (row group l>>4, column l&15): the
        // 16-bit field q of the two ballots is the word of row
        // mt2*16 + q*4 + reg; lane l < 32 keeps the word of row l
        unsigned long long m0 = __ballot(p0);
        unsigned long long m1 = __ballot(p1);
        int q = (lane >> 2) & 3;
        unsigned int w =
            (unsigned int)((m0 >> (q * 16)) & 0xFFFFull)
            | ((unsigned int)((m1 >> (q * 16)) & 0xFFFFull) << 16);
        if ((lane >> 4) == mt2 && (lane & 3) == reg) row_mask = w;
        v0 = p0 ? v0 : (__bf16)0.0f;
        v1 = p1 ? v1 : (__bf16)0.0f;
      }
      int64_t kk = row0 + row_base + reg;
      if (kk < K) {
        out[kk * 32 + col0] = v0;
        out[kk * 32 + 16 + col0] = v1;
      }
    }
  }
  if constexpr (RELU) {
    int64_t kk = row0 + wave * 32 + lane;
    if (lane < 32 && kk < K) mask[kk] = row_mask;
  }
}

__global__ __launch_bounds__(256)
void conv1_fwd_v3_kernel(const unsigned char* __restrict__ frames,
                         const __bf16* __restrict__ weight,
                         const float* __restrict__ bias,
                         __bf16* __restrict__ out, int64_t K,
                         float scale) {
  conv1_fwd_v3_body<false>(frames, weight, bias, out, nullptr, K, scale);
}

__global__ __launch_bounds__(256)
void conv1_fwd_v3_relu_kernel(const unsigned char* __restrict__ frames,
                              const __bf16* __restrict__ weight,
                              const float* __restrict__ bias,
                              __bf16* __restrict__ out,
                              unsigned int* __restrict__ mask, int64_t K,
                              float scale) {
  conv1_fwd_v3_body<true>(frames, weight, bias, out, mask, K, scale);
}

// =====================================================================
// v4 forward: frame-resident, persistent workgroups.
//
// v3 spends its time on work the result does not need: every 128-row
// workgroup (128 000 per step at batch 40960) restages the 16 KB
// weight image, every pixel is fetched and dequantised once per patch
// row it belongs to (the 8x8/stride-4 patches overlap 2x2), and each
// workgroup runs eight barrier pairs around 32 MFMAs per wave.
//
// Here a workgroup owns whole frames (grid-stride loop over the batch):
// - the 16 weight fragments (8 patch rows x 2 n-tiles) are read ONCE
//   per workgroup and live in registers (64 VGPRs);
// - a frame arrives as 1764 coalesced 16-byte loads, each pixel is
//   dequantised once and the frame is kept in LDS as a bf16 NHWC image
//   (56 448 B, two workgroups per CU);
// - the A fragment of output position (oh, ow), patch row pr, quarter
//   q is ONE aligned ds_read_b128 straight from that image: k = q*8+j
//   is pixel ow*4 + q*2 + j/4, channel j%4 of image row oh*4 + pr,
//   eight contiguous bf16;
// - the next frame's seven 16-byte loads per thread are issued before
//   the current frame's MFMAs, so they complete under them;
// - two barriers per FRAME: image written -> fragments read -> image
//   may be overwritten.
// Same MFMA instruction, operand roles, k-slot assignment, pr order
// and epilogue as v3, so the output and the mask are bit-identical.
// =====================================================================
#define FWD4_FRAME_ELEMS (84 * 84 * CONV1_CIN)   // 28224 u8 per frame
#define FWD4_CHUNKS (FWD4_FRAME_ELEMS / 16)      // 1764 16-byte loads
#define FWD4_LOADS ((FWD4_CHUNKS + 255) / 256)   // 7 per thread
#define FWD4_TILES (CONV1_POS / 16)              // 25 m-tiles per frame
#define FWD4_ROW_ELEMS (84 * CONV1_CIN)          // one image row

template <bool RELU>
__device__ __forceinline__
void conv1_fwd_v4_body(const unsigned char* __restrict__ frames,
                       const __bf16* __restrict__ weight,  // [256][32]
                       const float* __restrict__ bias,
                       __bf16* __restrict__ out,
                       unsigned int* __restrict__ mask, int64_t B,
                       float scale) {
  __shared__ __attribute__((aligned(16))) __bf16 s_f[FWD4_FRAME_ELEMS];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / MA_WAVE);
  const int lane = tid % MA_WAVE;
  const int col0 = lane & 15;
  const int k0 = (lane >> 4) * 8;

  // B fragments: lane holds W[pr*32 + k0 + j][h*16 + col0], j = 0..7
  bf16x8 wf[CONV1_KSZ][2];
#pragma unroll
  for (int pr = 0; pr < CONV1_KSZ; ++pr) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const __bf16* w = weight + (pr * 32 + k0 + j) * 32 + col0;
      wf[pr][0][j] = w[0];
      wf[pr][1][j] = w[16];
    }
  }
  const float bias0 = bias != nullptr ? bias[col0] : 0.0f;
  const float bias1 = bias != nullptr ? bias[16 + col0] : 0.0f;

  uint4 raw[FWD4_LOADS];
  auto load_frame = [&](int64_t f) {
    const uint4* src = (const uint4*)(frames + f * FWD4_FRAME_ELEMS);
#pragma unroll
    for (int i = 0; i < FWD4_LOADS; ++i) {
      int idx = tid + i * 256;
      // only the last of the seven rounds runs past the frame
      if (i < FWD4_LOADS - 1 || idx < FWD4_CHUNKS) raw[i] = src[idx];
    }
  };

  int64_t f = blockIdx.x;
  if (f < B) load_frame(f);
  for (; f < B; f += gridDim.x) {
    // dequantise the prefetched frame once, into the LDS image
#pragma unroll
    for (int i = 0; i < FWD4_LOADS; ++i) {
      int idx = tid + i * 256;
      if (i < FWD4_LOADS - 1 || idx < FWD4_CHUNKS) {
        unsigned int words[4] = {raw[i].x, raw[i].y, raw[i].z, raw[i].w};
        bf16x8 q0, q1;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            q0[w * 4 + j] = u8_bf16((words[w] >> (8 * j)) & 0xFF, scale);
            q1[w * 4 + j] =
                u8_bf16((words[w + 2] >> (8 * j)) & 0xFF, scale);
          }
        }
        *(bf16x8*)(s_f + idx * 16) = q0;
        *(bf16x8*)(s_f + idx * 16 + 8) = q1;
      }
    }
    __syncthreads();  // image of frame f complete
    if (f + gridDim.x < B) load_frame(f + gridDim.x);

    __bf16* out_f = out + f * (CONV1_POS * 32);
    for (int t = wave; t < FWD4_TILES; t += 4) {
      const int pos = t * 16 + col0;
      const int oh = pos / CONV1_OHW, ow = pos - oh * CONV1_OHW;
      const __bf16* a_ptr =
          s_f + (oh * CONV1_STRIDE * 84 + ow * CONV1_STRIDE) * CONV1_CIN
          + k0;
      f32x4 acc0 = (f32x4)(0.0f), acc1 = (f32x4)(0.0f);
#pragma unroll
      for (int pr = 0; pr < CONV1_KSZ; ++pr) {
        bf16x8 a_frag = *(const bf16x8*)(a_ptr + pr * FWD4_ROW_ELEMS);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag, wf[pr][0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag, wf[pr][1], acc1, 0, 0, 0);
      }
      // epilogue as v3 (C/D map: col=lane&15, row=(lane>>4)*4+reg)
      const int row_base = t * 16 + (lane >> 4) * 4;
      unsigned int row_mask = 0u;  // lanes 0..15: word of row t*16+lane
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        __bf16 v0 = (__bf16)(acc0[reg] + bias0);
        __bf16 v1 = (__bf16)(acc1[reg] + bias1);
        if constexpr (RELU) {
          // !(v <= 0) keeps NaN, as ATen's relu does
          bool p0 = !((float)v0 <= 0.0f);
          bool p1 = !((float)v1 <= 0.0f);
          // the 16-bit field q of the two ballots is the word of row
          // q*4 + reg of this tile; lane l < 16 keeps the word of row l
          unsigned long long m0 = __ballot(p0);
          unsigned long long m1 = __ballot(p1);
          int q = (lane >> 2) & 3;
          unsigned int w =
              (unsigned int)((m0 >> (q * 16)) & 0xFFFFull)
              | ((unsigned int)((m1 >> (q * 16)) & 0xFFFFull) << 16);
          if ((lane & 3) == reg) row_mask = w;
          v0 = p0 ? v0 : (__bf16)0.0f;
          v1 = p1 ? v1 : (__bf16)0.0f;
        }
        out_f[(row_base + reg) * 32 + col0] = v0;
        out_f[(row_base + reg) * 32 + 16 + col0] = v1;
      }
      if constexpr (RELU) {
        if (lane < 16) mask[f * CONV1_POS + t * 16 + lane] = row_mask;
      }
    }
    __syncthreads();  // all fragment reads of frame f done
  }
}

__global__ __launch_bounds__(256)
void conv1_fwd_v4_kernel(const unsigned char* __restrict__ frames,
                         const __bf16* __restrict__ weight,
                         const float* __restrict__ bias,
                         __bf16* __restrict__ out, int64_t B,
                         float scale) {
  conv1_fwd_v4_body<false>(frames, weight, bias, out, nullptr, B, scale);
}

__global__ __launch_bounds__(256)
void conv1_fwd_v4_relu_kernel(const unsigned char* __restrict__ frames,
                              const __bf16* __restrict__ weight,
                              const float* __restrict__ bias,
                              __bf16* __restrict__ out,
                              unsigned int* __restrict__ mask, int64_t B,
                              float scale) {
  conv1_fwd_v4_body<true>(frames, weight, bias, out, mask, B, scale);
}

// CU count of the current device, queried once per device
static int conv1_cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) dev = 0;
  if (cached[dev] == 0) {
    int n = 0;
    HIP_CHECK(hipDeviceGetAttribute(
        &n, hipDeviceAttributeMultiprocessorCount, dev));
    cached[dev] = n > 0 ? n : 1;
  }
  return cached[dev];
}

// Launches the frame-resident forward (mask == nullptr: plain kernel).
// Returns false without launching when its preconditions do not hold
// (whole frames, 16-byte aligned frame base); the caller then runs v3.
bool conv1_fwd_v4_launch(const unsigned char* frames, const void* weight,
                         const float* bias, void* out, unsigned int* mask,
                         bool relu, int64_t K, float scale,
                         hipStream_t stream) {
  if (K <= 0 || K % CONV1_POS != 0) return false;
  if ((uintptr_t)frames % 16 != 0) return false;
  const int64_t B = K / CONV1_POS;
  // 56 KB of LDS per workgroup: two resident workgroups per CU. The
  // grid is twice that, so that a CU which finishes early picks up
  // another workgroup (0.533 against 0.551 ms at batch 40960, spread
  // 0.005 ms; one workgroup per frame costs 0.64 ms)
  int64_t grid = (int64_t)conv1_cu_count() * 4;
  if (const char* e = getenv("MACHIN_CONV1_FWD_WG")) grid = atol(e);
  if (grid < 1) grid = 1;
  if (grid > B) grid = B;
  if (relu) {
    hipLaunchKernelGGL(conv1_fwd_v4_relu_kernel, dim3((unsigned)grid),
                       dim3(256), 0, stream, frames,
                       (const __bf16*)weight, bias, (__bf16*)out, mask, B,
                       scale);
  } else {
    hipLaunchKernelGGL(conv1_fwd_v4_kernel, dim3((unsigned)grid),
                       dim3(256), 0, stream, frames,
                       (const __bf16*)weight, bias, (__bf16*)out, B,
                       scale);
  }
  HIP_CHECK(hipGetLastError());
  return true;
}

// =====================================================================
// v4 weight gradient: frame-resident, no per-chunk transposition of x.
//
// v3 is bound by VALU issue (about 100 VALU instructions per MFMA):
// 64-bit divisions per 4-byte frame load, and every pixel fetched,
// dequantised and register-transposed once per patch it belongs to.
//
// Here a workgroup owns whole frames. Within one image row R the
// im2col element of output column ow, patch column kw, channel ci is
// row[ow*16 + kw*4 + ci]: with e = w*4 + ci the byte index in the row,
// n' = e & 15 and ow' = e >> 4, patch columns 0..3 of position ow are
// (n', ow' = ow) and patch columns 4..7 are (n' , ow' = ow + 1). So the
// row is stored ONCE, transposed at staging time, as T[R][n'][ow']
// (u8, ow' padded 21 -> 24), and
//   dW[co][pr][n']      = sum_{oh,ow'} dy [oh][ow'][co] * T[oh*4+pr][n'][ow']
//   dW[co][pr][16 + n'] = sum_{oh,ow'} dys[oh][ow'][co] * T[oh*4+pr][n'][ow']
// with dys[oh][ow'] = dy[oh][ow' - 1] (zero at ow' = 0) and dy zero
// for ow' >= 20. One B fragment (8 consecutive ow' of one (R, n'): one
// ds_read_b64, dequantised in registers) feeds four MFMAs: two m-tiles
// times {dy, dys}. The k-slots of an MFMA are positions: quarter q of
// k-step s is the pair (oh, ow' group of 8) number s*4 + q, 60 pairs =
// 15 k-steps per frame; positions inside a frame are small counters,
// there is no division by 400 anywhere.
//
// dy is kept transposed as Dt[co][oh][24] bf16 (masked as it is written,
// pads zero). The dys fragment is the dy fragment shifted by one
// element: four v_alignbit with the dword in front of it, which is the
// zero pad of the previous row for ow' = 0.
//
// Frames and dy arrive with 16- and 8-byte loads issued for frame f+1
// before the MFMAs of frame f; each thread transposes 4x4 byte blocks
// (x) and 8x4 bf16 blocks (dy) in registers on the way into LDS.
// LDS: T 84*408 + Dt (8 + 32*488)*2 = 65 520 B, two workgroups per CU.
// Wave w owns patch rows 2w and 2w+1: 2 pr x 2 halves x 2 m-tiles =
// 8 accumulator tiles. Split-K epilogue as v3.
// =====================================================================
#define WRW4_T_ROW 408       // bytes per image row of T: 16 n' x 24 + pad
#define WRW4_T_N 24          // bytes per (R, n')
#define WRW4_DT_CO 488       // elements per channel of Dt: 20 x 24 + 8
#define WRW4_DT_LEAD 8       // zero elements in front of channel 0
#define WRW4_KSTEPS 15       // 20 rows x 3 groups of 8 / 4 quarters
#define WRW4_X_TASKS (84 * 6)       // (row, 4 chunks of 16 B)
#define WRW4_DY_TASKS (20 * 3 * 8)  // (oh, ow' group, 4 channels)

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

__device__ __forceinline__ unsigned int byte_perm(unsigned int hi,
                                                  unsigned int lo,
                                                  unsigned int sel) {
  // result byte i = byte sel[i] of {hi, lo} (lo = bytes 0..3)
  return __builtin_amdgcn_perm(hi, lo, sel);
}

// 0xFFFFFFFF if bit `bit` of w is set, else 0
__device__ __forceinline__ unsigned int bit_fill(unsigned int w, int bit) {
  return (unsigned int)((int)(w << (31 - bit)) >> 31);
}

__device__ __forceinline__ bf16x8 u8x8_bf16(uint2 r, float scale) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = u8_bf16((r.x >> (8 * j)) & 0xFF, scale);
    v[4 + j] = u8_bf16((r.y >> (8 * j)) & 0xFF, scale);
  }
  return v;
}

template <bool MASKED>
__device__ __forceinline__
void conv1_wrw_v4_body(const __bf16* __restrict__ dy,
                       const unsigned int* __restrict__ mask,
                       const unsigned char* __restrict__ frames,
                       float* __restrict__ out,
                       float* __restrict__ b_out, int64_t B,
                       int64_t frames_per_wg, float scale) {
  __shared__ __attribute__((aligned(16)))
      unsigned char s_t[84 * WRW4_T_ROW];
  __shared__ __attribute__((aligned(16)))
      __bf16 s_dy[WRW4_DT_LEAD + CONV1_COUT * WRW4_DT_CO];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / MA_WAVE);
  const int lane = tid % MA_WAVE;
  const int n16 = lane & 15;   // m of the A fragment, n' of the B one
  const int q = lane >> 4;

  // zero the pads nobody writes again: the lead and the 8 elements
  // behind every channel (the dword in front of row 0 lies there)
  if (tid <= CONV1_COUT) {
    u32x4 z = {0u, 0u, 0u, 0u};
    int at = tid == 0 ? 0
                      : WRW4_DT_LEAD + (tid - 1) * WRW4_DT_CO
                            + CONV1_OHW * 24;
    *(u32x4*)(s_dy + at) = z;
  }

  // ---- staging tasks of this thread (fixed for the whole kernel) ----
  // x: task (R, h) loads chunks 4h..4h+3 of image row R (21 per row)
  int x_src[2], x_dst[2];
  bool x_on[2], x_tail[2];
  // dy: task (oh, g, cg) loads channels cg*4..+3 of positions g*8..+7
  int dy_src[2], dy_dst[2], dy_pos[2];
  bool dy_on[2], dy_tail[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    int task = tid + r * 256;
    int R = task / 6, h = task - R * 6;
    x_on[r] = task < WRW4_X_TASKS;
    x_tail[r] = h == 5;  // only chunk 20 exists
    x_src[r] = R * FWD4_ROW_ELEMS + h * 64;
    x_dst[r] = R * WRW4_T_ROW + h * 4;
    int cg = task & 7, rest = task >> 3;
    int oh = rest / 3, g = rest - oh * 3;
    dy_on[r] = task < WRW4_DY_TASKS;
    dy_tail[r] = g == 2;  // positions 20..23 do not exist
    dy_pos[r] = oh * CONV1_OHW + g * 8;
    dy_src[r] = dy_pos[r] * CONV1_COUT + cg * 4;
    dy_dst[r] = WRW4_DT_LEAD + cg * 4 * WRW4_DT_CO + oh * 24 + g * 8;
  }

  uint4 xr[2][4];
  uint2 dr[2][8];
  uint4 mlo[2], mhi[2];
  auto load_frame = [&](int64_t f) {
    const unsigned char* xf = frames + f * FWD4_FRAME_ELEMS;
    const __bf16* df = dy + f * (CONV1_POS * CONV1_COUT);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xr[r][i] = make_uint4(0u, 0u, 0u, 0u);
        if (x_on[r] && (i == 0 || !x_tail[r])) {
          xr[r][i] = *(const uint4*)(xf + x_src[r] + i * 16);
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        dr[r][i] = make_uint2(0u, 0u);
        if (dy_on[r] && (i < 4 || !dy_tail[r])) {
          dr[r][i] = *(const uint2*)(df + dy_src[r] + i * CONV1_COUT);
        }
      }
      if constexpr (MASKED) {
        // 16-byte aligned: 400*f + 20*oh + 8*g words
        const unsigned int* mf = mask + f * CONV1_POS + dy_pos[r];
        mlo[r] = make_uint4(0u, 0u, 0u, 0u);
        mhi[r] = make_uint4(0u, 0u, 0u, 0u);
        if (dy_on[r]) {
          mlo[r] = *(const uint4*)mf;
          if (!dy_tail[r]) mhi[r] = *(const uint4*)(mf + 4);
        }
      }
    }
  };
  auto store_frame = [&]() {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (x_on[r]) {
        unsigned int in[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          in[i][0] = xr[r][i].x; in[i][1] = xr[r][i].y;
          in[i][2] = xr[r][i].z; in[i][3] = xr[r][i].w;
        }
#pragma unroll
        for (int dw = 0; dw < 4; ++dw) {
          // 4x4 byte transpose: out j = byte j of chunks 0..3
          unsigned int lo01 = byte_perm(in[1][dw], in[0][dw], 0x05010400u);
          unsigned int hi01 = byte_perm(in[1][dw], in[0][dw], 0x07030602u);
          unsigned int lo23 = byte_perm(in[3][dw], in[2][dw], 0x05010400u);
          unsigned int hi23 = byte_perm(in[3][dw], in[2][dw], 0x07030602u);
          unsigned int c[4] = {byte_perm(lo23, lo01, 0x05040100u),
                               byte_perm(lo23, lo01, 0x07060302u),
                               byte_perm(hi23, hi01, 0x05040100u),
                               byte_perm(hi23, hi01, 0x07060302u)};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            *(unsigned int*)(s_t + x_dst[r] + (dw * 4 + j) * WRW4_T_N) =
                c[j];
          }
        }
      }
      if (dy_on[r]) {
        unsigned int dx[8], dyv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          dx[i] = dr[r][i].x;
          dyv[i] = dr[r][i].y;
        }
        if constexpr (MASKED) {
          unsigned int mw[8] = {mlo[r].x, mlo[r].y, mlo[r].z, mlo[r].w,
                                mhi[r].x, mhi[r].y, mhi[r].z, mhi[r].w};
          const int c0 = ((tid + r * 256) & 7) * 4;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            unsigned int bits = mw[i] >> c0;
            dx[i] &= (bit_fill(bits, 0) & 0x0000FFFFu)
                     | (bit_fill(bits, 1) & 0xFFFF0000u);
            dyv[i] &= (bit_fill(bits, 2) & 0x0000FFFFu)
                      | (bit_fill(bits, 3) & 0xFFFF0000u);
          }
        }
        // channel j of 8 positions: dword d = positions 2d, 2d+1
        u32x4 o[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          o[0][d] = byte_perm(dx[2 * d + 1], dx[2 * d], 0x05040100u);
          o[1][d] = byte_perm(dx[2 * d + 1], dx[2 * d], 0x07060302u);
          o[2][d] = byte_perm(dyv[2 * d + 1], dyv[2 * d], 0x05040100u);
          o[3][d] = byte_perm(dyv[2 * d + 1], dyv[2 * d], 0x07060302u);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          *(u32x4*)(s_dy + dy_dst[r] + j * WRW4_DT_CO) = o[j];
        }
      }
    }
  };

  f32x4 acc[2][2][2];  // [pr of this wave][half][m-tile]
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      acc[a][b][0] = (f32x4)(0.0f);
      acc[a][b][1] = (f32x4)(0.0f);
    }
  }
  float bias_acc[2] = {0.0f, 0.0f};

  const int64_t f_begin = (int64_t)blockIdx.x * frames_per_wg;
  const int64_t f_end = min(f_begin + frames_per_wg, B);

  if (f_begin < f_end) load_frame(f_begin);
  for (int64_t f = f_begin; f < f_end; ++f) {
    store_frame();
    __syncthreads();  // images of frame f complete
    if (f + 1 < f_end) load_frame(f + 1);

#pragma unroll 3
    for (int s = 0; s < WRW4_KSTEPS; ++s) {
      const int p = s * 4 + q;
      const int oh = p / 3, g = p - oh * 3;
      const __bf16* ap =
          s_dy + WRW4_DT_LEAD + n16 * WRW4_DT_CO + oh * 24 + g * 8;
      const unsigned char* bp =
          s_t + (oh * CONV1_STRIDE + wave * 2) * WRW4_T_ROW
          + n16 * WRW4_T_N + g * 8;
      u32x4 a[2];
      unsigned int prev[2];
      uint2 braw[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        a[mt] = *(const u32x4*)(ap + mt * 16 * WRW4_DT_CO);
        prev[mt] = *(const unsigned int*)(ap + mt * 16 * WRW4_DT_CO - 2);
      }
      braw[0] = *(const uint2*)bp;
      braw[1] = *(const uint2*)(bp + WRW4_T_ROW);
      bf16x8 af[2], as[2], bf[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        u32x4 sh;
        sh[0] = __builtin_amdgcn_alignbit(a[mt][0], prev[mt], 16);
        sh[1] = __builtin_amdgcn_alignbit(a[mt][1], a[mt][0], 16);
        sh[2] = __builtin_amdgcn_alignbit(a[mt][2], a[mt][1], 16);
        sh[3] = __builtin_amdgcn_alignbit(a[mt][3], a[mt][2], 16);
        af[mt] = __builtin_bit_cast(bf16x8, a[mt]);
        as[mt] = __builtin_bit_cast(bf16x8, sh);
      }
      bf[0] = u8x8_bf16(braw[0], scale);
      bf[1] = u8x8_bf16(braw[1], scale);
      // fused bias: the waves take turns at summing the dy fragments
      if ((s & 3) == wave) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
          for (int j = 0; j < 8; ++j) bias_acc[mt] += (float)af[mt][j];
        }
      }
#pragma unroll
      for (int prl = 0; prl < 2; ++prl) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          acc[prl][0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mt], bf[prl], acc[prl][0][mt], 0, 0, 0);
          acc[prl][1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              as[mt], bf[prl], acc[prl][1][mt], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // all fragment reads of frame f done
  }

  // ---- epilogue: split-K atomics (C/D map: col=lane&15,
  // row=(lane>>4)*4+reg) ----------------------------------------------
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    float b = bias_acc[mt];
    b += __shfl_down(b, 32, 64);
    b += __shfl_down(b, 16, 64);
    if (lane < 16) atomicAdd(&b_out[mt * 16 + lane], b);
  }
#pragma unroll
  for (int prl = 0; prl < 2; ++prl) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        int col = (wave * 2 + prl) * 32 + half * 16 + n16;
        int row_base = mt * 16 + q * 4;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          atomicAdd(&out[(row_base + reg) * CONV1_N + col],
                    acc[prl][half][mt][reg]);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256)
void conv1_wrw_v4_kernel(const __bf16* __restrict__ dy,
                         const unsigned char* __restrict__ frames,
                         float* __restrict__ out,
                         float* __restrict__ b_out, int64_t B,
                         int64_t frames_per_wg, float scale) {
  conv1_wrw_v4_body<false>(dy, nullptr, frames, out, b_out, B,
                           frames_per_wg, scale);
}

__global__ __launch_bounds__(256)
void conv1_wrw_v4_masked_kernel(const __bf16* __restrict__ dy,
                                const unsigned int* __restrict__ mask,
                                const unsigned char* __restrict__ frames,
                                float* __restrict__ out,
                                float* __restrict__ b_out, int64_t B,
                                int64_t frames_per_wg, float scale) {
  conv1_wrw_v4_body<true>(dy, mask, frames, out, b_out, B, frames_per_wg,
                          scale);
}

// Launches the frame-resident weight-gradient kernel into the zeroed
// scratch (mask == nullptr: unmasked). Returns false without launching
// when its preconditions do not hold; the caller then runs v3.
bool conv1_wrw_v4_launch(const void* dy, const unsigned int* mask,
                         const unsigned char* frames, float* scratch,
                         float* grad_b, int64_t K, int64_t target_wg,
                         float scale, hipStream_t stream) {
  if (K <= 0 || K % CONV1_POS != 0) return false;
  if ((uintptr_t)frames % 16 != 0 || (uintptr_t)dy % 8 != 0 ||
      (uintptr_t)mask % 16 != 0) {
    return false;
  }
  const int64_t B = K / CONV1_POS;
  if (target_wg < 1) target_wg = 1;
  int64_t frames_per_wg = (B + target_wg - 1) / target_wg;
  int grid = (int)((B + frames_per_wg - 1) / frames_per_wg);
  if (mask != nullptr) {
    hipLaunchKernelGGL(conv1_wrw_v4_masked_kernel, dim3(grid), dim3(256),
                       0, stream, (const __bf16*)dy, mask, frames, scratch,
                       grad_b, B, frames_per_wg, scale);
  } else {
    hipLaunchKernelGGL(conv1_wrw_v4_kernel, dim3(grid), dim3(256), 0,
                       stream, (const __bf16*)dy, frames, scratch, grad_b,
                       B, frames_per_wg, scale);
  }
  HIP_CHECK(hipGetLastError());
  return true;
}

// fused-activation entry points (v3 and v4 kernels only)
void conv1_fwd_relu_launch(const unsigned char* frames, const void* weight,
                           const float* bias, void* out,
                           unsigned int* mask, int64_t K, float scale,
                           hipStream_t stream) {
  const char* ver = getenv("MACHIN_CONV1_V");
  int v = ver ? atoi(ver) : 4;
  if (v != 3 && conv1_fwd_v4_launch(frames, weight, bias, out, mask, true,
                                    K, scale, stream)) {
    return;
  }
  int64_t grid = (K + FWD3_ROWS - 1) / FWD3_ROWS;
  hipLaunchKernelGGL(conv1_fwd_v3_relu_kernel, dim3((unsigned)grid),
                     dim3(256), 0, stream, frames, (const __bf16*)weight,
                     bias, (__bf16*)out, mask, K, scale);
  HIP_CHECK(hipGetLastError());
}

void conv1_wrw_masked_launch(const void* dy, const unsigned int* mask,
                             const unsigned char* frames, float* scratch,
                             float* grad_w, float* grad_b, int64_t K,
                             float scale, hipStream_t stream) {
  HIP_CHECK(hipMemsetAsync(scratch, 0,
                           CONV1_COUT * CONV1_N * sizeof(float), stream));
  HIP_CHECK(hipMemsetAsync(grad_b, 0, CONV1_COUT * sizeof(float),
                           stream));
  int64_t target_wg = 2048;
  if (const char* e = getenv("MACHIN_CONV1_WG")) target_wg = atol(e);
  const char* ver = getenv("MACHIN_CONV1_V");
  int v = ver ? atoi(ver) : 4;
  if (v != 3 && conv1_wrw_v4_launch(dy, mask, frames, scratch, grad_b, K,
                                    target_wg, scale, stream)) {
    hipLaunchKernelGGL(conv1_wrw_reorder_kernel,
                       dim3((CONV1_COUT * CONV1_N + 255) / 256), dim3(256),
                       0, stream, scratch, grad_w);
    HIP_CHECK(hipGetLastError());
    return;
  }
  if (target_wg < 1) target_wg = 1;
  int64_t k_per_wg = (K + target_wg - 1) / target_wg;
  k_per_wg = ((k_per_wg + KC3 - 1) / KC3) * KC3;
  if (k_per_wg < KC3) k_per_wg = KC3;
  int grid = (int)((K + k_per_wg - 1) / k_per_wg);
  hipLaunchKernelGGL(conv1_wrw_v3_masked_kernel, dim3(grid), dim3(256), 0,
                     stream, (const __bf16*)dy, mask, frames, scratch,
                     grad_b, K, k_per_wg, scale);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(conv1_wrw_reorder_kernel,
                     dim3((CONV1_COUT * CONV1_N + 255) / 256), dim3(256),
                     0, stream, scratch, grad_w);
  HIP_CHECK(hipGetLastError());
}
