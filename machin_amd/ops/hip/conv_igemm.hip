// gfx950 implicit-GEMM convolution for the two Nature-CNN layers the
// library used to run: conv2 (32 -> 64, 4x4, stride 2) and conv3
// (64 -> 64, 3x3, stride 1), forward with a fused bias + ReLU epilogue
// and the gradient with respect to the input. bf16 NHWC, no padding,
// dilation 1, groups 1; N, H and W are runtime values.
// Semantics: machin_amd.ops.fused_conv._ConvBiasReLUIgemmFn.
//
// One kernel body serves both directions, because both are the same
// computation: a small stride-CS window of TH x TW taps slides over an
// image that is resident in LDS, and every tap contributes CK channels
// to the reduction.
//
//   forward        image = x[n] (H x W x Cin), window KH x KW, step S,
//                  K = KH KW Cin, out = Cout channels at (oy, ox).
//   data gradient  image = g[n] (OH x OW x Cout) inside a ring of
//                  T - 1 zero pixels (T = KH / S), window T x T, step 1.
//                  dx[S a + py, S b + px, ci] =
//                    sum_{j, i < T, co} gpad[a + j, b + i, co]
//                                       * W[co, ci, py + S (T-1-j),
//                                                   px + S (T-1-i)]
//                  for each of the S x S parity classes (py, px): every
//                  row of a class runs the same K = T T Cout loop, the
//                  ring makes the range test disappear, and input rows
//                  or columns that no tap reaches ((H - KH) % S != 0)
//                  come out of the ring as exact zeros. The resident
//                  image has ceil(H / S) + T - 1 rows so that those
//                  rows index it in bounds.
//
// Instruction: v_mfma_f32_16x16x32_bf16, fragment layout as pinned in
// the header of noisy_linear_mfma.hip. Because CK % 32 == 0 one k-step
// is 32 consecutive channels of one tap, so an image fragment is ONE
// 16-byte LDS read per lane, straight from the resident image at
//   ((y0 + ty) * IW + x0 + tx) * PITCH + 32 c + 8 (lane >> 4),
// pixel = lane & 15 of the tile; no im2col tile is ever written. A
// pixel's CK channels are kept PITCH = CK + 8 elements apart: with the
// natural 64- or 128-byte pitch the 16 pixels of a fragment read would
// share two or four LDS banks, 16 bytes of padding spread them.
//
// Operand roles: the weights are the MFMA's first operand (m = output
// channel) and the image its second (n = pixel), so a lane ends up
// with FOUR CONSECUTIVE CHANNELS of ONE pixel: D[4 (l >> 4) + reg]
// [l & 15]. In a channels-last row that is one 8-byte write.
//
// Weights: a "unit" is (parity class, 16 output channels). Each of the
// four waves owns units / 4 of them and keeps their K x 16 weight
// slices in registers for the kernel's lifetime: 64 VGPRs for conv2
// (forward: 16 fragments of one unit; data gradient: 8 fragments each
// of two classes), 72 for conv3. The wrapper hands the weights over as
// [class][out channel][K], K running (tap row, tap column, channel) as
// the image does, so a fragment is one 16-byte global load. LDS then
// serves image fragments only.
//
// Workgroups are persistent: each loops over groups of G samples (G as
// many as fit the two 32 KB LDS buffers). The 16-byte global loads of
// the next group are issued into registers (8 per thread) right after
// the barrier that completes the current image and are written to LDS
// at the top of the next round, as the v4 stem forward does. Rows are
// the group's flat (sample, a, b) pixels of a class cut into 16-row
// tiles; tiles may straddle samples, only a class's last tile is
// partial (its spare rows read the last valid pixel and are dropped at
// the write).
//
// Epilogue: forward relu(bf16(acc + bias)), fp32 bias, ONE rounding,
// the project's ReLU (s <= 0 ? +0 : s, NaN kept); data gradient
// bf16(acc). Results go to a second LDS buffer that holds the group's
// output exactly as global memory will (channels-last rows, or for
// EPI == flat the [sample][channel][pixel] NCHW-flattened matrix the fc
// layer reads); after one barrier the buffer leaves as a linear run of
// 16-byte stores. Two barriers per group.
//
// No atomics; every sum has a fixed order: two calls return equal bits.
// Bounds: the launchers admit a shape only if G >= 1 samples fit both
// buffers, loads and stores are limited by the group's sample count,
// and a window never leaves its sample's resident image (forward:
// (OH-1) S + KH <= H; data gradient: a + T - 1 <= ceil(H/S) + T - 2).
#include "common.h"
#include "conv_igemm.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
// 16 bytes as a native vector: an array of these is promoted to
// registers, one of HIP's uint4 structs is copied through scratch memory
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

#define CIG_BUF 32768    // bytes of each LDS buffer (image, output)
#define CIG_THREADS 256
#define CIG_PF 8         // prefetch registers: 8 x 256 x 16 B = CIG_BUF

enum { CIG_ROWS = 0, CIG_FLAT = 1, CIG_SCATTER = 2 };

struct cig_args {
  const __bf16* in;    // [N][gh][gw][CK]
  const __bf16* w;     // [OS*OS][NOUT][K]
  const float* bias;   // [NOUT], forward only
  __bf16* out;         // [N][oh][ow][NOUT], or [N][NOUT][oh*ow] (flat)
  int64_t N;
  int G;               // samples per group
  int gh, gw;          // one sample's image in global memory
  int ih, iw;          // the resident image: that image inside its ring
  int oh, ow;          // one sample's whole output image
};

template <int TH, int TW, int CS, int OS, int CK, int NOUT, int EPI>
__global__ __launch_bounds__(CIG_THREADS) void cig_kernel(cig_args args) {
  constexpr int PAD = EPI == CIG_SCATTER ? TH - 1 : 0;
  constexpr int K = TH * TW * CK;
  constexpr int KS = K / 32;             // MFMA k-steps
  constexpr int NT = NOUT / 16;          // channel tiles
  constexpr int UPW = OS * OS * NT / 4;  // units per wave
  constexpr int CPP = CK / 8;            // 16-byte chunks per pixel
  constexpr int PITCH = CK + 8;          // LDS elements between pixels
  static_assert(CK % 32 == 0 && NOUT % 16 == 0 && (OS * OS * NT) % 4 == 0,
                "geometry does not fit the unit split");
  // kernel arguments as plain locals, so that nothing takes the address
  // of the argument block
  const __bf16* __restrict__ a_in = args.in;
  const __bf16* __restrict__ a_w = args.w;
  const float* __restrict__ a_bias = args.bias;
  __bf16* __restrict__ a_out = args.out;
  const int64_t nn = args.N;
  const int ng = args.G;
  const int gh = args.gh, gw = args.gw, ih = args.ih, iw = args.iw;
  const int oh = args.oh, ow = args.ow;

  __shared__ __attribute__((aligned(16))) __bf16 s_img[CIG_BUF / 2];
  __shared__ __attribute__((aligned(16))) __bf16 s_out[CIG_BUF / 2];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / MA_WAVE);
  const int lane = tid % MA_WAVE;
  const int l15 = lane & 15;  // weights: channel of the tile; image: pixel
  const int q = lane >> 4;

  // weight fragments: lane holds w[cls][nt*16 + l15][32 ks + 8 q + j]
  bf16x8 wf[UPW][KS];
  float bias4[UPW][4];
#pragma unroll
  for (int u = 0; u < UPW; ++u) {
    const int unit = wave + 4 * u;
    const int cls = unit / NT, nt = unit % NT;
    const __bf16* wrow =
        a_w + (int64_t)(cls * NOUT + nt * 16 + l15) * K + 8 * q;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      wf[u][ks] = *reinterpret_cast<const bf16x8*>(wrow + ks * 32);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      bias4[u][reg] =
          EPI == CIG_SCATTER ? 0.0f : a_bias[nt * 16 + 4 * q + reg];
  }

  const int in_pix = gh * gw;          // pixels of one global image
  const int in_chunks = in_pix * CPP;      // 16-byte chunks of it
  const int out_pix = oh * ow;
  const int64_t groups = (nn + ng - 1) / ng;

  auto group_count = [&](int64_t grp) {
    const int64_t left = nn - grp * ng;
    return (int)(left < ng ? left : ng);
  };

  u32x4 raw[CIG_PF];
  auto load_group = [&](int64_t grp) {
    const u32x4* src = reinterpret_cast<const u32x4*>(
        a_in + grp * ng * (int64_t)in_pix * CK);
    const int n = group_count(grp) * in_chunks;
#pragma unroll
    for (int i = 0; i < CIG_PF; ++i) {
      // past the group's end the last chunk is read again
      const int idx = tid + i * CIG_THREADS;
      raw[i] = src[idx < n ? idx : n - 1];
    }
  };
  auto stage_group = [&](int cnt) {
    const int n = cnt * in_chunks;
#pragma unroll
    for (int i = 0; i < CIG_PF; ++i) {
      // a register past the end holds the last chunk again and writes
      // it to the same place again: equal bytes, no branch
      int idx = tid + i * CIG_THREADS;
      idx = idx < n ? idx : n - 1;
      int pix = idx / CPP;
      const int c = idx % CPP;
      if constexpr (PAD > 0) {
        // pixel -> (sample, y, x) -> inside the ring
        const int s = pix / in_pix, r = pix - s * in_pix;
        const int y = r / gw, x = r - y * gw;
        pix = (s * ih + y + PAD) * iw + x + PAD;
      }
      *reinterpret_cast<u32x4*>(s_img + pix * PITCH + c * 8) = raw[i];
    }
  };

  if constexpr (PAD > 0) {
    // the ring is written once: staging only ever touches the interior
    for (int i = tid; i < CIG_BUF / 16; i += CIG_THREADS)
      reinterpret_cast<u32x4*>(s_img)[i] = (u32x4)(0u);
    __syncthreads();
  }

  int64_t grp = blockIdx.x;
  if (grp < groups) load_group(grp);
  for (; grp < groups; grp += gridDim.x) {
    const int cnt = group_count(grp);
    stage_group(cnt);
    __syncthreads();  // image of this group complete
    if (grp + gridDim.x < groups) load_group(grp + gridDim.x);

#pragma unroll
    for (int u = 0; u < UPW; ++u) {
      const int unit = wave + 4 * u;
      const int cls = unit / NT, nt = unit % NT;
      const int py = cls / OS, px = cls % OS;
      // this class's pixels of one sample: ca x cb
      const int ca = (oh - py + OS - 1) / OS;
      const int cb = (ow - px + OS - 1) / OS;
      const int cpix = ca * cb;
      const int rows = cnt * cpix;
      for (int r0 = 0; r0 < rows; r0 += 16) {
        const bool ok = r0 + l15 < rows;
        const int r = ok ? r0 + l15 : rows - 1;
        const int s = r / cpix, rem = r - s * cpix;
        const int a = rem / cb, b = rem - a * cb;
        const __bf16* ap =
            s_img + ((s * ih + a * CS) * iw + b * CS) * PITCH + 8 * q;
        f32x4 acc = (f32x4)(0.0f);
#pragma unroll
        for (int ty = 0; ty < TH; ++ty)
#pragma unroll
          for (int tx = 0; tx < TW; ++tx)
#pragma unroll
            for (int c = 0; c < CK / 32; ++c) {
              const bf16x8 af = *reinterpret_cast<const bf16x8*>(
                  ap + (ty * iw + tx) * PITCH + c * 32);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  wf[u][(ty * TW + tx) * (CK / 32) + c], af, acc, 0, 0, 0);
            }
        if (!ok) continue;
        bf16x4 v;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          __bf16 e = (__bf16)(acc[reg] + bias4[u][reg]);
          if constexpr (EPI != CIG_SCATTER) {
            // NaN fails the test and is kept; -0 becomes +0
            if ((float)e <= 0.0f) e = (__bf16)0.0f;
          }
          v[reg] = e;
        }
        const int oy = OS * a + py, ox = OS * b + px;
        const int ch = nt * 16 + 4 * q;
        if constexpr (EPI == CIG_FLAT) {
          __bf16* o = s_out + (s * NOUT + ch) * out_pix + oy * ow + ox;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) o[reg * out_pix] = v[reg];
        } else {
          *reinterpret_cast<bf16x4*>(
              s_out + ((s * oh + oy) * ow + ox) * NOUT + ch) = v;
        }
      }
    }
    __syncthreads();  // image reads done, output image complete

    u32x4* dst = reinterpret_cast<u32x4*>(
        a_out + grp * ng * (int64_t)out_pix * NOUT);
    const int n = cnt * out_pix * (NOUT / 8);
    for (int i = tid; i < n; i += CIG_THREADS)
      dst[i] = reinterpret_cast<const u32x4*>(s_out)[i];
    // the next round writes s_out only after its first barrier, which
    // every thread reaches after this copy
  }
}

// CU count of the current device, queried once per device
static int cig_cu_count() {
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

// 64 KB of LDS per workgroup: two resident workgroups per CU, and the
// grid is that many. MACHIN_CONV_IGEMM_WG overrides it (read per call).
unsigned cig_grid(int64_t groups) {
  int64_t grid = (int64_t)cig_cu_count() * 2;
  if (const char* e = getenv("MACHIN_CONV_IGEMM_WG")) grid = atol(e);
  if (grid < 1) grid = 1;
  if (grid > groups) grid = groups;
  return (unsigned)grid;
}

// Index of the layer in the table (conv_igemm.h), -1 for anything else.
int conv_igemm_geometry(int64_t cin, int64_t cout, int64_t ksize,
                        int64_t stride) {
  for (int i = 0; i < CIG_NGEOM; ++i) {
    const cig_geom g = CIG_GEOM[i];
    if (cin == g.cin && cout == g.cout && ksize == g.ksize &&
        stride == g.stride)
      return i;
  }
  return -1;
}

// Samples per group of the forward (bwd = 0) or the data gradient
// (bwd = 1) on H x W inputs: as many as fit both LDS buffers, 0 when
// not even one does (or the shape is not a valid convolution).
int conv_igemm_group(int geom, int64_t H, int64_t W, int bwd) {
  if (geom < 0 || geom >= CIG_NGEOM) return 0;
  const cig_geom g = CIG_GEOM[geom];
  if (H < g.ksize || W < g.ksize || H > 4096 || W > 4096) return 0;
  const int64_t OH = (H - g.ksize) / g.stride + 1;
  const int64_t OW = (W - g.ksize) / g.stride + 1;
  int64_t img, out;
  if (!bwd) {
    img = H * W * (g.cin + 8) * 2;  // PITCH
    out = OH * OW * g.cout * 2;
  } else {
    const int64_t T = g.ksize / g.stride;
    const int64_t ih = (H + g.stride - 1) / g.stride + T - 1;
    const int64_t iw = (W + g.stride - 1) / g.stride + T - 1;
    img = ih * iw * (g.cout + 8) * 2;
    out = H * W * g.cin * 2;
  }
  const int64_t big = img > out ? img : out;
  return (int)(CIG_BUF / big);
}

// Launches the instantiation of table entry GI: the forward (EPI rows or
// flat: window k x k, step S, one class) or the data gradient (EPI
// scatter: window k/S x k/S over the ringed gradient image, step 1,
// S x S classes, channel roles swapped).
template <int GI, int EPI>
static void cig_launch(const cig_args& a, hipStream_t stream) {
  constexpr cig_geom g = CIG_GEOM[GI];
  constexpr bool bwd = EPI == CIG_SCATTER;
  constexpr int T = bwd ? g.ksize / g.stride : g.ksize;
  const int64_t groups = (a.N + a.G - 1) / a.G;
  hipLaunchKernelGGL(
      (cig_kernel<T, T, bwd ? 1 : g.stride, bwd ? g.stride : 1,
                  bwd ? g.cout : g.cin, bwd ? g.cin : g.cout, EPI>),
      dim3(cig_grid(groups)), dim3(CIG_THREADS), 0, stream, a);
  HIP_CHECK(hipGetLastError());
}

// y = relu(bf16(conv(x, w) + bias)); x [N, H, W, Cin] bf16, w
// [1][Cout][KH*KW*Cin] bf16, bias [Cout] fp32; out is channels-last
// rows [N*OH*OW, Cout], or with flat the [N, Cout*OH*OW] matrix.
void conv_igemm_fwd_launch(int geom, const void* x, const void* w,
                           const float* bias, void* out, int64_t N, int H,
                           int W, int flat, hipStream_t stream) {
  const int G = conv_igemm_group(geom, H, W, 0);
  if (G < 1) throw std::runtime_error("conv_igemm_fwd: shape not eligible");
  if (N <= 0) return;
  const cig_geom g = CIG_GEOM[geom];
  cig_args a;
  a.in = (const __bf16*)x, a.w = (const __bf16*)w, a.bias = bias;
  a.out = (__bf16*)out, a.N = N, a.G = G;
  a.gh = a.ih = H, a.gw = a.iw = W;
  a.oh = (H - g.ksize) / g.stride + 1, a.ow = (W - g.ksize) / g.stride + 1;
  if (geom == 0) {
    if (flat) cig_launch<0, CIG_FLAT>(a, stream);
    else cig_launch<0, CIG_ROWS>(a, stream);
  } else {
    if (flat) cig_launch<1, CIG_FLAT>(a, stream);
    else cig_launch<1, CIG_ROWS>(a, stream);
  }
}

// dx [N, H, W, Cin] = data gradient of the conv for g [N, OH, OW, Cout]
// bf16; w is the class repack [S*S][Cin][T*T*Cout] (see the header).
void conv_igemm_bwd_data_launch(int geom, const void* gy, const void* w,
                                void* dx, int64_t N, int H, int W,
                                hipStream_t stream) {
  const int G = conv_igemm_group(geom, H, W, 1);
  if (G < 1)
    throw std::runtime_error("conv_igemm_bwd_data: shape not eligible");
  if (N <= 0) return;
  const cig_geom g = CIG_GEOM[geom];
  const int T = g.ksize / g.stride;
  cig_args a;
  a.in = (const __bf16*)gy, a.w = (const __bf16*)w, a.bias = nullptr;
  a.out = (__bf16*)dx, a.N = N, a.G = G;
  a.gh = (H - g.ksize) / g.stride + 1, a.gw = (W - g.ksize) / g.stride + 1;
  a.ih = (H + g.stride - 1) / g.stride + T - 1;
  a.iw = (W + g.stride - 1) / g.stride + T - 1;
  a.oh = H, a.ow = W;
  if (geom == 0) cig_launch<0, CIG_SCATTER>(a, stream);
  else cig_launch<1, CIG_SCATTER>(a, stream);
}
