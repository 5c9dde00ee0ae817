// gfx950 batched PixelCatch: step and render thousands of envs in one
// launch, frames written straight into HBM.
//
// PixelCatch (machin_amd/env/envs/pixel_catch.py) is an integer
// function of three small numbers per frame: paddle x, ball x, ball y.
// Per env the device keeps
//   state[e] = {paddle_x, ball_x, ball_y, balls_left, steps, done,
//               hist0, hist1, hist2, hist3}                    int32
//   ball_no[e]                                                 int64
// where hist* is the 4-entry frame history, newest last, each entry
// packed as paddle_x | ball_x << 8 | ball_y << 16 | valid << 24. The
// observation stack is RENDERED from the history and never read back,
// so a step is a pure write stream: 28 KB of stack + 7 KB of newest
// plane per env (+ 7 KB, or 35 KB on an episode's first step, when
// the episode is recorded).
//
// One step of env e is PixelCatchEnv.step followed by the optional
// reset (semantics in ops.pixelcatch_step's docstring). A new ball's x
// is 3 + philox4x32_10(key = seed, counter = (ball_no, e))[0] % 78,
// i.e. ma_philox4(seed, subseq = e, offset = ball_no).
//
// Work decomposition: one 256-thread workgroup per env, grid capped at
// 2048 blocks and grid-strided over envs. Every lane reads the env's
// 12 state words (made wave-uniform with readfirstlane, so the update
// runs on the scalar unit), a barrier follows, lane 0 writes the new
// state. Every store is 16 bytes:
//   plane / NCHW: 441 x 16 flat pixels per plane (the four planes of
//                 a stack as one flat run of 1764);
//   NHWC:         1764 x (4 pixels x 4 planes) per env.
// A chunk whose rows hold neither a ball nor the paddle (most of them)
// is stored as zeros without looking at single pixels. Pixels are
// decided by comparisons only: no state value is ever used as an
// address, so no state content can make the kernel write outside its
// buffers (the log slot, the one exception, is range-checked).
// No LDS, no atomics, no scratch.
#include "common.h"

typedef unsigned char u8;
typedef uint32_t u32;

#define PC_H 84
#define PC_W 84
#define PC_HW (PC_H * PC_W)        // 7056 = 441 * 16
#define PC_CHUNKS (PC_HW / 16)     // 441 uint4 per plane
#define PC_QUADS (PC_HW / 4)       // 1764 uint4 per NHWC stack
#define PC_K 4
#define PC_NSTATE 10
#define PC_BLOCK 256
#define PC_PADDLE_ROW (PC_H - 3)   // 81: first paddle row, landing line

struct pc_args {
  int32_t* __restrict__ state;        // [E, 10]
  int64_t* __restrict__ ball_no;      // [E]
  const int64_t* __restrict__ action; // [E]            (step only)
  const u8* __restrict__ mask;        // [E]            (reset only)
  uint4* __restrict__ obs;            // [E, 4, 84, 84] / channels_last
  uint4* __restrict__ frame;          // [E, 84, 84]
  float* __restrict__ reward;         // [E]
  float* __restrict__ done;           // [E]
  int32_t* __restrict__ ep_len;       // [E]
  uint4* __restrict__ log_frames;     // [E, max_len + 4, 84, 84] or null
  int64_t* __restrict__ log_action;   // [E, max_len]
  float* __restrict__ log_reward;     // [E, max_len]
  float* __restrict__ log_terminal;   // [E, max_len]
  int64_t E;
  uint64_t seed;
  int balls, max_steps, max_len;
  bool auto_reset, nhwc;
};

__device__ __forceinline__ int pc_uniform(int v) {
  return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ int pc_pack(int px, int bx, int by) {
  return (px & 255) | ((bx & 255) << 8) | ((by & 255) << 16) | (1 << 24);
}

// one history entry, unpacked; an invalid entry renders as zeros
struct pc_sprite {
  int px, bx, by, valid;
};

__device__ __forceinline__ pc_sprite pc_unpack(int h) {
  pc_sprite s;
  s.px = h & 255;
  s.bx = (h >> 8) & 255;
  s.by = (h >> 16) & 255;
  s.valid = (h >> 24) & 1;
  return s;
}

// does row r hold any lit pixel of s?
__device__ __forceinline__ bool pc_row_lit(const pc_sprite& s, int r) {
  return s.valid && (r >= PC_PADDLE_ROW || (r >= s.by - 1 && r <= s.by + 1));
}

// PixelCatchEnv._frame: paddle rows 81..83, columns [px-4, px+4); ball
// rows [by-1, by+1], columns [bx-1, bx+1]; the clipping to the screen
// is implied because (r, c) is always a screen pixel.
__device__ __forceinline__ u32 pc_pixel(const pc_sprite& s, int r, int c) {
  const bool paddle = r >= PC_PADDLE_ROW && c >= s.px - 4 && c < s.px + 4;
  const bool ball = r >= s.by - 1 && r <= s.by + 1 && c >= s.bx - 1 &&
                    c <= s.bx + 1;
  return (s.valid && (paddle || ball)) ? 255u : 0u;
}

// four flat pixels p .. p + 3 of the plane of sprite s, as one word
__device__ __forceinline__ u32 pc_word(pc_sprite s, int p) {
  u32 w = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = (p + q) / PC_W;
    w |= pc_pixel(s, r, p + q - r * PC_W) << (8 * q);
  }
  return w;
}

// chunk c (16 flat pixels) of the plane of sprite s
__device__ __forceinline__ uint4 pc_chunk(pc_sprite s, int c) {
  const int p0 = c * 16;
  const int r = p0 / PC_W;
  // 16 flat pixels touch rows r and (at most) r + 1
  if (!(pc_row_lit(s, r) || pc_row_lit(s, r + 1)))
    return make_uint4(0u, 0u, 0u, 0u);
  return make_uint4(pc_word(s, p0), pc_word(s, p0 + 4), pc_word(s, p0 + 8),
                    pc_word(s, p0 + 12));
}

// one plane [84, 84] as 441 dwordx4 stores
__device__ __forceinline__ void pc_render_plane(uint4* __restrict__ dst,
                                                int packed) {
  const pc_sprite s = pc_unpack(packed);
  for (int c = threadIdx.x; c < PC_CHUNKS; c += PC_BLOCK)
    dst[c] = pc_chunk(s, c);
}

// four consecutive planes [4, 84, 84] as one flat run of 1764 dwordx4
// stores (7 passes of the block instead of 4 x 2 with ragged tails)
// (the entries come by value: a select over array elements would be
// turned into a dynamically indexed private array)
__device__ __forceinline__ void pc_render_planes4(uint4* __restrict__ dst,
                                                  int h0, int h1, int h2,
                                                  int h3) {
  for (int i = threadIdx.x; i < PC_QUADS; i += PC_BLOCK) {
    const int j = i / PC_CHUNKS;
    const int h = j == 0 ? h0 : j == 1 ? h1 : j == 2 ? h2 : h3;
    dst[i] = pc_chunk(pc_unpack(h), i - j * PC_CHUNKS);
  }
}

// the NHWC stack [84, 84, 4] as 1764 dwordx4 stores: 4 pixels of one
// row (84 % 4 == 0) x 4 planes per store
__device__ __forceinline__ void pc_render_nhwc(uint4* __restrict__ dst,
                                               const int hist[PC_K]) {
  pc_sprite s[PC_K];
#pragma unroll
  for (int j = 0; j < PC_K; ++j) s[j] = pc_unpack(hist[j]);
  for (int i = threadIdx.x; i < PC_QUADS; i += PC_BLOCK) {
    const int p0 = i * 4;
    const int r = p0 / PC_W;
    const int col = p0 - r * PC_W;
    u32 w[4] = {0u, 0u, 0u, 0u};
    if (pc_row_lit(s[0], r) || pc_row_lit(s[1], r) || pc_row_lit(s[2], r) ||
        pc_row_lit(s[3], r)) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int j = 0; j < PC_K; ++j)
          w[q] |= pc_pixel(s[j], r, col + q) << (8 * j);
      }
    }
    dst[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

__device__ __forceinline__ void pc_render_obs(const pc_args& a, int64_t e,
                                              const int hist[PC_K]) {
  uint4* dst = a.obs + e * (int64_t)PC_QUADS;  // 4 planes = 1764 uint4
  if (a.nhwc) {
    pc_render_nhwc(dst, hist);
  } else {
    pc_render_planes4(dst, hist[0], hist[1], hist[2], hist[3]);
  }
}

// ball_x of ball number `no` of env e, in [3, 81)
__device__ __forceinline__ int pc_spawn_x(uint64_t seed, int64_t e,
                                          int64_t no) {
  uint32_t r[4];
  ma_philox4(seed, (uint64_t)e, (uint64_t)no, r);
  return 3 + (int)(r[0] % 78u);
}

struct pc_env {
  int px, bx, by, balls_left, steps, done;
  int hist[PC_K];
  int64_t ball_no;
};

// every lane loads the same words; readfirstlane makes them SGPRs
__device__ __forceinline__ pc_env pc_load(const pc_args& a, int64_t e) {
  const int32_t* s = a.state + e * PC_NSTATE;
  pc_env v;
  v.px = pc_uniform(s[0]);
  v.bx = pc_uniform(s[1]);
  v.by = pc_uniform(s[2]);
  v.balls_left = pc_uniform(s[3]);
  v.steps = pc_uniform(s[4]);
  v.done = pc_uniform(s[5]);
#pragma unroll
  for (int j = 0; j < PC_K; ++j) v.hist[j] = pc_uniform(s[6 + j]);
  const int64_t no = a.ball_no[e];
  const u32 lo = (u32)pc_uniform((int)(u32)no);
  const u32 hi = (u32)pc_uniform((int)(u32)((uint64_t)no >> 32));
  v.ball_no = (int64_t)(((uint64_t)hi << 32) | lo);
  return v;
}

__device__ __forceinline__ void pc_save(const pc_args& a, int64_t e,
                                        const pc_env& v) {
  int32_t* s = a.state + e * PC_NSTATE;
  s[0] = v.px;
  s[1] = v.bx;
  s[2] = v.by;
  s[3] = v.balls_left;
  s[4] = v.steps;
  s[5] = v.done;
#pragma unroll
  for (int j = 0; j < PC_K; ++j) s[6 + j] = v.hist[j];
  a.ball_no[e] = v.ball_no;
}

// PixelCatchEnv.reset: centred paddle, a new ball, history = three
// invalid entries + the first frame
__device__ __forceinline__ void pc_reset(const pc_args& a, int64_t e,
                                         pc_env& v) {
  v.px = PC_W / 2;
  v.balls_left = a.balls;
  v.steps = 0;
  v.done = 0;
  v.bx = pc_spawn_x(a.seed, e, v.ball_no);
  v.ball_no += 1;
  v.by = 0;
  v.hist[0] = v.hist[1] = v.hist[2] = 0;
  v.hist[3] = pc_pack(v.px, v.bx, v.by);
}

__global__ __launch_bounds__(PC_BLOCK) void pixelcatch_step_kernel(pc_args a) {
  const bool lane0 = threadIdx.x == 0;
  for (int64_t e = blockIdx.x; e < a.E; e += gridDim.x) {
    pc_env v = pc_load(a, e);
    // the host env raises on actions outside {0, 1, 2}; a kernel
    // cannot raise without a sync, so it clamps
    const int64_t raw = a.action[e];
    const int act = pc_uniform(raw < 0 ? 0 : (raw > 2 ? 2 : (int)raw));
    // all lanes have read state[e]; lane 0 may write it from here on
    __syncthreads();
    if (!a.auto_reset && v.done) {
      // latched: nothing but reward 0 / done 1 changes
      if (lane0) {
        a.reward[e] = 0.0f;
        a.done[e] = 1.0f;
        a.ep_len[e] = 0;
      }
      continue;
    }
    const int s_idx = v.steps;  // index of this step inside its episode
    int old_hist[PC_K];
#pragma unroll
    for (int j = 0; j < PC_K; ++j) old_hist[j] = v.hist[j];

    int px = v.px + (act - 1) * 3;
    v.px = px < 4 ? 4 : (px > PC_W - 4 ? PC_W - 4 : px);
    v.by += 3;
    float rew = 0.0f;
    bool dn = false;
    if (v.by >= PC_PADDLE_ROW) {
      const int d = v.bx - v.px;
      rew = (d <= 5 && d >= -5) ? 1.0f : -1.0f;
      v.balls_left -= 1;
      if (v.balls_left <= 0) {
        dn = true;
      } else {
        v.bx = pc_spawn_x(a.seed, e, v.ball_no);
        v.ball_no += 1;
        v.by = 0;
      }
    }
    v.steps += 1;
    if (v.steps >= a.max_steps) dn = true;
    const int newest = pc_pack(v.px, v.bx, v.by);
    v.hist[0] = old_hist[1];
    v.hist[1] = old_hist[2];
    v.hist[2] = old_hist[3];
    v.hist[3] = newest;
    const int length = v.steps;

    pc_render_plane(a.frame + e * (int64_t)PC_CHUNKS, newest);
    if (a.log_frames != nullptr && s_idx >= 0 && s_idx < a.max_len) {
      uint4* lf = a.log_frames +
                  e * (int64_t)(a.max_len + PC_K) * (int64_t)PC_CHUNKS;
      if (s_idx == 0)
        pc_render_planes4(lf, old_hist[0], old_hist[1], old_hist[2],
                          old_hist[3]);
      pc_render_plane(lf + (int64_t)(PC_K + s_idx) * PC_CHUNKS, newest);
      if (lane0) {
        const int64_t row = e * (int64_t)a.max_len + s_idx;
        a.log_action[row] = act;
        a.log_reward[row] = rew;
        a.log_terminal[row] = dn ? 1.0f : 0.0f;
      }
    }
    v.done = dn ? 1 : 0;
    if (dn && a.auto_reset) pc_reset(a, e, v);
    pc_render_obs(a, e, v.hist);
    if (lane0) {
      pc_save(a, e, v);
      a.reward[e] = rew;
      a.done[e] = dn ? 1.0f : 0.0f;
      a.ep_len[e] = dn ? length : 0;
    }
  }
}

__global__ __launch_bounds__(PC_BLOCK) void pixelcatch_reset_kernel(pc_args a) {
  for (int64_t e = blockIdx.x; e < a.E; e += gridDim.x) {
    pc_env v = pc_load(a, e);
    const int m = pc_uniform((int)a.mask[e]);
    __syncthreads();
    if (m == 0) continue;
    pc_reset(a, e, v);
    pc_render_obs(a, e, v.hist);
    if (threadIdx.x == 0) pc_save(a, e, v);
  }
}

// ---------------------------------------------------------------------
// host-side drivers (called from bindings.cpp)
// ---------------------------------------------------------------------
static int pc_grid(int64_t E) {
  // one block per env, capped like ma_grid
  return ma_grid(E * PC_BLOCK, PC_BLOCK);
}

void pixelcatch_step_launch(int32_t* state, int64_t* ball_no,
                            const int64_t* action, unsigned char* obs,
                            unsigned char* frame, float* reward, float* done,
                            int32_t* ep_len, unsigned char* log_frames,
                            int64_t* log_action, float* log_reward,
                            float* log_terminal, int64_t E, uint64_t seed,
                            int balls, int max_steps, int max_len,
                            bool auto_reset, bool nhwc, hipStream_t stream) {
  if (E == 0) return;
  pc_args a;
  a.state = state;
  a.ball_no = ball_no;
  a.action = action;
  a.mask = nullptr;
  a.obs = (uint4*)obs;
  a.frame = (uint4*)frame;
  a.reward = reward;
  a.done = done;
  a.ep_len = ep_len;
  a.log_frames = (uint4*)log_frames;
  a.log_action = log_action;
  a.log_reward = log_reward;
  a.log_terminal = log_terminal;
  a.E = E;
  a.seed = seed;
  a.balls = balls;
  a.max_steps = max_steps;
  a.max_len = max_len;
  a.auto_reset = auto_reset;
  a.nhwc = nhwc;
  hipLaunchKernelGGL(pixelcatch_step_kernel, dim3(pc_grid(E)),
                     dim3(PC_BLOCK), 0, stream, a);
}

void pixelcatch_reset_launch(int32_t* state, int64_t* ball_no,
                             const unsigned char* mask, unsigned char* obs,
                             int64_t E, uint64_t seed, int balls, bool nhwc,
                             hipStream_t stream) {
  if (E == 0) return;
  pc_args a = {};
  a.state = state;
  a.ball_no = ball_no;
  a.mask = mask;
  a.obs = (uint4*)obs;
  a.E = E;
  a.seed = seed;
  a.balls = balls;
  a.nhwc = nhwc;
  hipLaunchKernelGGL(pixelcatch_reset_kernel, dim3(pc_grid(E)),
                     dim3(PC_BLOCK), 0, stream, a);
}
