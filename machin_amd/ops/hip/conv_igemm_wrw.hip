// gfx950 weight gradient of the two implicit-GEMM layers (conv_igemm.h):
// conv2 (32 -> 64, 4x4, stride 2) and conv3 (64 -> 64, 3x3, stride 1).
//   dW[co, ci, ky, kx] = bf16( sum_{n, oy, ox} g[n, oy, ox, co]
//                                            * x[n, S oy + ky, S ox + kx, ci] )
// g [N, OH, OW, Cout] and x [N, H, W, Cin] bf16 channels-last, fp32
// accumulation, ONE rounding; N, H and W are runtime values.
// Semantics: machin_amd.ops.fused_conv._ConvBiasReLUIgemmWrwFn.
//
// Formulation. The reduction index is the pixel, so both images are
// kept in LDS as channel-major planes on ONE common grid. With
// T = KH / S, PH x PW = ceil(H / S) x ceil(W / S) and p = a PW + b:
//
//   xplane_{py,px}[ci][p] = x[S a + py, S b + px, ci]   (0 where the
//                           pixel does not exist: ragged parity planes)
//   gpad[co][p]           = g[a, b, co] for a < OH and b < OW, else 0,
//                           with (T-1)(PW+1) zeros in front
//
//   dW[co, ci, S j + py, S i + px] =
//       sum_n sum_p gpad[n][co][p - (j PW + i)] * xplane_{py,px}[n][ci][p]
//
// The row wrap of a shifted read (b - i < 0) lands in columns
// >= PW - (T-1) >= OW, which are zero; a - j < 0 lands in the zeros in
// front. Input rows and columns that no tap reaches ((H - KH) % S != 0)
// meet zeros of gpad without a test. Samples of a group are laid end to
// end at pitch PP = PH PW with no rounding: the last non-zero of a
// sample's gpad is (OH-1) PW + OW - 1 <= PP - (T-1)(PW+1) - 1, so the
// tail of sample n IS the zero front of sample n + 1, and the reduction
// is one flat run of G PP positions cut into k-steps of 32 that may
// straddle samples. Only the run's end is rounded up to 32, with zeros
// on both sides. The price is MFMA work on padding: 100 positions for
// 81 output pixels on conv2, 81 for 49 on conv3, plus that rounding.
//
// Instruction: v_mfma_f32_16x16x32_bf16, fragment layout as pinned in
// the header of noisy_linear_mfma.hip. g is the first operand (m = co,
// k = position), x the second (n = ci): lane l gets
// D[co = 4 (l >> 4) + reg][ci = l & 15].
//   x fragment  ONE aligned 16-byte LDS read at row (class, ci),
//               position 32 ks + 8 (l >> 4); shared by the T T taps of
//               its class.
//   g fragment  the same read of row co at position
//               LEAD + 32 ks + 8 (l >> 4) - (j PW + i): two aligned
//               16-byte reads and a funnel shift by the wave-uniform
//               misalignment (LEAD - j PW - i) & 7: two levels of
//               dword selects and four v_alignbit. Shared by all
//               classes and ci tiles.
// Row pitches are multiples of 8 elements whose eighth is odd, so the
// 16 rows of a fragment read start in different banks.
//
// Work split: wave w of four owns output channels 16 w .. 16 w + 15 and
// for them the whole Cin x KH x KW tile: T T shifts x S S classes x
// Cin / 16 tiles = 32 accumulator tiles for conv2, 36 for conv3 (128
// and 144 registers), held for the kernel's lifetime. Per k-step a wave
// reads S S Cin / 16 x fragments (8 / 4) and T T g fragments (4 / 9)
// for 32 / 36 MFMAs. No im2col tile exists anywhere.
//
// Staging: a 16-byte global load is 8 channels of one pixel; it is
// transposed on its way into LDS as 8 two-byte writes into 8 channel
// rows. Where each load goes depends on its index in the group only,
// so the destinations are computed once, before the loop. Samples past
// the count of a ragged last group are written as zeros. Everything
// that is not a pixel is zeroed once and never written again.
//
// Workgroups are persistent and loop over groups of G samples (as many
// as fit the prefetch registers, 8 + 4 loads of 16 bytes per thread,
// and the 64 KB of LDS). The loads of the next group are issued right
// after the barrier that completes the current planes, before its
// MFMAs. Two barriers per group. Accumulators, prefetch registers and
// fragments together exceed 256 registers, so a wave takes the whole
// file of its SIMD (214 VGPRs + 128 AGPRs conv2, 211 + 144 conv3, no
// scratch): ONE workgroup per CU, and the second half of the 2 x CUs
// grid runs after the first.
//
// Split-K: each workgroup writes its fp32 tile once, at the end, to its
// own slab [grid][Cout][KH KW Cin]; ciw_reduce adds the slabs in slab
// order, rounds once to bf16 and writes [Cout, Cin, KH, KW]. No
// atomics; every sum has a fixed order: two calls with the same grid
// return equal bits.
// Bounds: the launcher admits a shape only if G >= 1; loads are clamped
// to the group's last chunk, LDS writes go to precomputed in-plane
// destinations, the last x read ends at 32 ksteps <= RPX and the last g
// read at LEAD + 32 ksteps + 8 <= RPG.
#include "common.h"
#include "conv_igemm.h"

#include <stdexcept>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

#define CIW_THREADS 256
#define CIW_LDS 65536  // bytes of LDS (the static limit)
#define CIW_PFX 8      // 16-byte prefetch registers for x
#define CIW_PFG 4      // and for g

struct ciw_plan {
  int G;         // samples per group, 0: not eligible
  int ph, pw;    // the common plane grid
  int lead;      // zeros in front of gpad, a multiple of 8
  int rpx, rpg;  // elements between channel rows of the x and g planes
};

struct ciw_args {
  const __bf16* g;  // [N][OH][OW][COUT]
  const __bf16* x;  // [N][H][W][CIN]
  float* slab;      // [grid][COUT][KH*KW*CIN]
  int64_t N;
  int H, W, OH, OW;
  ciw_plan p;
};

// elements r .. r + 7 of the sixteen in {lo, hi}; r is wave-uniform
__device__ __forceinline__ bf16x8 ciw_shift(u32x4 lo, u32x4 hi, int r) {
  const bool s2 = (r & 4) != 0, s1 = (r & 2) != 0;
  const unsigned t0 = s2 ? lo[2] : lo[0], t1 = s2 ? lo[3] : lo[1];
  const unsigned t2 = s2 ? hi[0] : lo[2], t3 = s2 ? hi[1] : lo[3];
  const unsigned t4 = s2 ? hi[2] : hi[0], t5 = s2 ? hi[3] : hi[1];
  const unsigned u0 = s1 ? t1 : t0, u1 = s1 ? t2 : t1, u2 = s1 ? t3 : t2;
  const unsigned u3 = s1 ? t4 : t3, u4 = s1 ? t5 : t4;
  const unsigned sh = (r & 1) * 16;
  u32x4 o;
  o[0] = __builtin_amdgcn_alignbit(u1, u0, sh);
  o[1] = __builtin_amdgcn_alignbit(u2, u1, sh);
  o[2] = __builtin_amdgcn_alignbit(u3, u2, sh);
  o[3] = __builtin_amdgcn_alignbit(u4, u3, sh);
  return __builtin_bit_cast(bf16x8, o);
}

template <int KS, int S, int CIN, int COUT>
__global__ __launch_bounds__(CIW_THREADS) void ciw_kernel(ciw_args args) {
  constexpr int T = KS / S, CLS = S * S, CT = CIN / 16;
  constexpr int CPX = CIN / 8, CPG = COUT / 8;  // 16-byte chunks per pixel
  constexpr int K = KS * KS * CIN;
  static_assert(COUT == 64 && CIN % 16 == 0 && KS % S == 0,
                "geometry does not fit the wave split");
  const __bf16* __restrict__ a_g = args.g;
  const __bf16* __restrict__ a_x = args.x;
  float* __restrict__ a_slab = args.slab;
  const int64_t nn = args.N;
  const int ng = args.p.G, pw = args.p.pw, pp = args.p.ph * args.p.pw;
  const int lead = args.p.lead, rpx = args.p.rpx, rpg = args.p.rpg;
  const int W = args.W, OW = args.OW;
  const int hw = args.H * args.W, ohw = args.OH * args.OW;

  __shared__ __attribute__((aligned(16))) unsigned short s_mem[CIW_LDS / 2];
  unsigned short* s_x = s_mem;                    // [CLS][CIN][rpx]
  unsigned short* s_g = s_mem + CLS * CIN * rpx;  // [COUT][rpg]

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / MA_WAVE);
  const int lane = tid % MA_WAVE;
  const int l15 = lane & 15;
  const int q = lane >> 4;

  // zeros everywhere; staging only ever writes pixels
  for (int i = tid; i < CIW_LDS / 16; i += CIW_THREADS)
    reinterpret_cast<u32x4*>(s_mem)[i] = (u32x4)(0u);

  // where this thread's loads go: chunk idx of a group is 8 channels of
  // pixel idx / CPX of the group; -1 past the G samples
  int xdst[CIW_PFX], gdst[CIW_PFG];
#pragma unroll
  for (int i = 0; i < CIW_PFX; ++i) {
    const int idx = tid + i * CIW_THREADS;
    const int pix = idx / CPX, c = idx % CPX;
    const int s = pix / hw, rem = pix - s * hw;
    const int y = rem / W, xx = rem - y * W;
    const int cls = (y % S) * S + xx % S;
    const int pos = s * pp + (y / S) * pw + xx / S;
    xdst[i] = s < ng ? (cls * CIN + 8 * c) * rpx + pos : -1;
  }
#pragma unroll
  for (int i = 0; i < CIW_PFG; ++i) {
    const int idx = tid + i * CIW_THREADS;
    const int pix = idx / CPG, c = idx % CPG;
    const int s = pix / ohw, rem = pix - s * ohw;
    const int oy = rem / OW, ox = rem - oy * OW;
    gdst[i] = s < ng ? 8 * c * rpg + lead + s * pp + oy * pw + ox : -1;
  }

  const int64_t groups = (nn + ng - 1) / ng;
  auto group_count = [&](int64_t grp) {
    const int64_t left = nn - grp * ng;
    return (int)(left < ng ? left : ng);
  };

  u32x4 rawx[CIW_PFX], rawg[CIW_PFG];
  auto load_group = [&](int64_t grp) {
    const int cnt = group_count(grp);
    const u32x4* sx = reinterpret_cast<const u32x4*>(
        a_x + grp * ng * (int64_t)hw * CIN);
    const u32x4* sg = reinterpret_cast<const u32x4*>(
        a_g + grp * ng * (int64_t)ohw * COUT);
    const int nx = cnt * hw * CPX, ngc = cnt * ohw * CPG;
    // past the group's end the last chunk is read and replaced by zeros
#pragma unroll
    for (int i = 0; i < CIW_PFX; ++i) {
      const int idx = tid + i * CIW_THREADS;
      const u32x4 v = sx[idx < nx ? idx : nx - 1];
      rawx[i] = idx < nx ? v : (u32x4)(0u);
    }
#pragma unroll
    for (int i = 0; i < CIW_PFG; ++i) {
      const int idx = tid + i * CIW_THREADS;
      const u32x4 v = sg[idx < ngc ? idx : ngc - 1];
      rawg[i] = idx < ngc ? v : (u32x4)(0u);
    }
  };
  auto stage_group = [&]() {
#pragma unroll
    for (int i = 0; i < CIW_PFX; ++i)
      if (xdst[i] >= 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          s_x[xdst[i] + e * rpx] =
              (unsigned short)(rawx[i][e >> 1] >> (16 * (e & 1)));
      }
#pragma unroll
    for (int i = 0; i < CIW_PFG; ++i)
      if (gdst[i] >= 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          s_g[gdst[i] + e * rpg] =
              (unsigned short)(rawg[i][e >> 1] >> (16 * (e & 1)));
      }
  };

  f32x4 acc[T * T][CLS][CT];
#pragma unroll
  for (int t = 0; t < T * T; ++t)
#pragma unroll
    for (int cls = 0; cls < CLS; ++cls)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[t][cls][ct] = (f32x4)(0.0f);

  const unsigned short* xrow = s_x + l15 * rpx + 8 * q;
  const unsigned short* grow = s_g + (16 * wave + l15) * rpg + 8 * q;

  int64_t grp = blockIdx.x;
  if (grp < groups) load_group(grp);
  __syncthreads();  // the zeros are in place
  for (; grp < groups; grp += gridDim.x) {
    const int cnt = group_count(grp);
    stage_group();
    __syncthreads();  // planes of this group complete
    if (grp + gridDim.x < groups) load_group(grp + gridDim.x);

    const int ksteps = (cnt * pp + 31) >> 5;
    for (int ks = 0; ks < ksteps; ++ks) {
      bf16x8 xf[CLS][CT];
#pragma unroll
      for (int cls = 0; cls < CLS; ++cls)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          xf[cls][ct] = *reinterpret_cast<const bf16x8*>(
              xrow + (cls * CIN + 16 * ct) * rpx + 32 * ks);
#pragma unroll
      for (int j = 0; j < T; ++j)
#pragma unroll
        for (int i = 0; i < T; ++i) {
          const int e0 = lead - (j * pw + i);  // >= 0, wave-uniform
          const unsigned short* gp = grow + 32 * ks + (e0 & ~7);
          const bf16x8 gf =
              ciw_shift(*reinterpret_cast<const u32x4*>(gp),
                        *reinterpret_cast<const u32x4*>(gp + 8), e0 & 7);
#pragma unroll
          for (int cls = 0; cls < CLS; ++cls)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
              acc[j * T + i][cls][ct] =
                  __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                      gf, xf[cls][ct], acc[j * T + i][cls][ct], 0, 0, 0);
        }
    }
    __syncthreads();  // plane reads done before the next staging
  }

  // this workgroup's slab: [co][(ky, kx, ci)]
  float* slab = a_slab + (int64_t)blockIdx.x * COUT * K;
#pragma unroll
  for (int j = 0; j < T; ++j)
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
      for (int cls = 0; cls < CLS; ++cls)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int ky = S * j + cls / S, kx = S * i + cls % S;
          float* o = slab + (16 * wave + 4 * q) * K + (ky * KS + kx) * CIN +
                     16 * ct + l15;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)
            o[reg * K] = acc[j * T + i][cls][ct][reg];
        }
}

// dW[co][ci][tap] = bf16(slab 0 + slab 1 + ...), one thread per element
__global__ __launch_bounds__(64) void ciw_reduce(
    const float* __restrict__ slab, __bf16* __restrict__ dw, int slabs,
    int cout, int cin, int taps) {
  const int total = cout * taps * cin;
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= total) return;
  float s = 0.0f;
  for (int i = 0; i < slabs; ++i) s += slab[(int64_t)i * total + e];
  const int co = e / (taps * cin), k = e % (taps * cin);
  dw[(co * cin + k % cin) * taps + k / cin] = (__bf16)s;
}

static int ciw_odd8(int64_t n) {  // >= n, a multiple of 8, eighth odd
  return (int)((((n + 7) / 8) | 1) * 8);
}

// The LDS layout and the samples per group of the weight gradient on
// H x W inputs: as many as fit the prefetch registers and the LDS; G = 0
// when not even one does (or the shape is not a valid convolution).
static ciw_plan ciw_make_plan(int geom, int64_t H, int64_t W) {
  ciw_plan p = {0, 0, 0, 0, 0, 0};
  if (geom < 0 || geom >= CIG_NGEOM) return p;
  const cig_geom g = CIG_GEOM[geom];
  if (H < g.ksize || W < g.ksize || H > 4096 || W > 4096) return p;
  const int64_t OH = (H - g.ksize) / g.stride + 1;
  const int64_t OW = (W - g.ksize) / g.stride + 1;
  const int64_t T = g.ksize / g.stride, cls = g.stride * g.stride;
  p.ph = (int)((H + g.stride - 1) / g.stride);
  p.pw = (int)((W + g.stride - 1) / g.stride);
  p.lead = (int)(((T - 1) * (p.pw + 1) + 7) / 8 * 8);
  const int64_t gx = CIW_PFX * CIW_THREADS / (H * W * (g.cin / 8));
  const int64_t gg = CIW_PFG * CIW_THREADS / (OH * OW * (g.cout / 8));
  for (int64_t G = gx < gg ? gx : gg; G >= 1; --G) {
    const int64_t kl = (G * p.ph * p.pw + 31) / 32 * 32;
    p.rpx = ciw_odd8(kl);
    p.rpg = ciw_odd8(p.lead + kl + 8);
    if ((cls * g.cin * p.rpx + (int64_t)g.cout * p.rpg) * 2 <= CIW_LDS) {
      p.G = (int)G;
      break;
    }
  }
  return p;
}

int conv_igemm_wrw_group(int geom, int64_t H, int64_t W) {
  return ciw_make_plan(geom, H, W).G;
}

// Number of slabs conv_igemm_wrw_launch will write for N samples.
int64_t conv_igemm_wrw_slabs(int geom, int64_t N, int64_t H, int64_t W) {
  const int G = conv_igemm_wrw_group(geom, H, W);
  if (G < 1 || N <= 0) return 0;
  return cig_grid((N + G - 1) / G);
}

// dW [Cout, Cin, k, k] bf16 for g [N, OH, OW, Cout] and x [N, H, W, Cin]
// bf16; slab is fp32 scratch of `slabs` x Cout x k*k*Cin elements, slabs
// as conv_igemm_wrw_slabs returned it (the grid is not sized again here,
// so a change of the environment between the two cannot outrun the
// allocation).
void conv_igemm_wrw_launch(int geom, const void* gy, const void* x,
                           float* slab, int64_t slabs, void* dw, int64_t N,
                           int H, int W, hipStream_t stream) {
  const ciw_plan p = ciw_make_plan(geom, H, W);
  if (p.G < 1) throw std::runtime_error("conv_igemm_wrw: shape not eligible");
  if (N <= 0) return;
  const int64_t groups = (N + p.G - 1) / p.G;
  if (slabs < 1 || slabs > groups)
    throw std::runtime_error("conv_igemm_wrw: bad slab count");
  const cig_geom g = CIG_GEOM[geom];
  ciw_args a;
  a.g = (const __bf16*)gy, a.x = (const __bf16*)x, a.slab = slab, a.N = N;
  a.H = H, a.W = W;
  a.OH = (H - g.ksize) / g.stride + 1, a.OW = (W - g.ksize) / g.stride + 1;
  a.p = p;
  if (geom == 0) {
    constexpr cig_geom c = CIG_GEOM[0];
    hipLaunchKernelGGL((ciw_kernel<c.ksize, c.stride, c.cin, c.cout>),
                       dim3((unsigned)slabs), dim3(CIW_THREADS), 0, stream, a);
  } else {
    constexpr cig_geom c = CIG_GEOM[1];
    hipLaunchKernelGGL((ciw_kernel<c.ksize, c.stride, c.cin, c.cout>),
                       dim3((unsigned)slabs), dim3(CIW_THREADS), 0, stream, a);
  }
  HIP_CHECK(hipGetLastError());
  const int total = g.cout * g.ksize * g.ksize * g.cin;
  hipLaunchKernelGGL(ciw_reduce, dim3((total + 63) / 64), dim3(64), 0, stream,
                     slab, (__bf16*)dw, (int)slabs, g.cout, g.cin,
                     g.ksize * g.ksize);
  HIP_CHECK(hipGetLastError());
}
