// Python bindings for the machin_amd gfx950 kernels — written
// directly against PyTorch-ROCm's native HIP API (the
// "masquerading-as-CUDA" device layer every ROCm extension runs on),
// so the tree carries NO hipify-generated sources.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstdint>
#include <vector>

using at::Tensor;

// launchers defined in the .hip translation units
void sumtree_update_launch(float*, const int64_t*, const float*, int64_t,
                           int64_t, int, hipStream_t);
void sumtree_build_launch(float*, int64_t, hipStream_t);
void sumtree_sample_launch(const float*, const float*, int64_t*, int64_t,
                           int64_t, int, int64_t, hipStream_t);
void discounted_returns_launch(const float*, const float*, const float*,
                               float*, int64_t, int64_t, float, hipStream_t);
void gae_launch(const float*, const float*, const float*, const float*,
                float*, int64_t, int64_t, float, float, hipStream_t);
void vtrace_launch(const float*, const float*, const float*, const float*,
                   const float*, const float*, float*, float*, int64_t,
                   int64_t, float, float, float, float, hipStream_t);
void nstep_returns_launch(const float*, const float*, float*, int64_t,
                          int64_t, float, int, hipStream_t);
void vtrace_bt_launch(const float*, const float*, const float*,
                      const float*, const float*, const float*, float*,
                      float*, int64_t, int64_t, float, float, float,
                      float, hipStream_t);
void categorical_projection_launch(const float*, const float*, const float*,
                                   float*, int64_t, int64_t, float, float,
                                   float, hipStream_t);
void c51_loss_fwd_launch(const void*, const int64_t*, const void*,
                         const void*, const float*, const float*,
                         const float*, float, float*, float*, int64_t*,
                         float*, float*, int64_t, int, int, float, float,
                         bool, bool, hipStream_t);
void c51_loss_bwd_launch(const void*, const int64_t*, const float*,
                         const float*, const float*, const float*, void*,
                         int64_t, int, int, bool, bool, hipStream_t);
void multi_tensor_polyak_launch(void*, const int64_t*, int64_t, int64_t,
                                float, hipStream_t);
void fused_rmsprop_launch(void*, const int64_t*, int64_t, int64_t,
                          float*, float, float, float, float,
                          hipStream_t);
void gaussian_sample_logprob_launch(const float*, const float*, float*,
                                    float*, int64_t, int64_t, uint64_t,
                                    uint64_t, int, float, hipStream_t);
void gaussian_logprob_launch(const float*, const float*, const float*,
                             float*, int64_t, int64_t, int, float,
                             hipStream_t);
void normal_noise_launch(float*, int64_t, float, float, uint64_t, uint64_t,
                         int, hipStream_t);
void ou_update_launch(float*, int64_t, float, float, float, float, uint64_t,
                      uint64_t, hipStream_t);
void u8_to_bf16_scale_launch(const unsigned char*, void*, int64_t, float,
                             hipStream_t);
void framestack_gather_launch(const unsigned char*, const int64_t*,
                              unsigned char*, unsigned char*, int64_t,
                              int64_t, int64_t, int, bool, hipStream_t);
void framestack_gather_nstep_launch(
    const unsigned char*, const int64_t*, const int64_t*, const float*,
    const float*, const int64_t*, unsigned char*, unsigned char*, float*,
    float*, int64_t*, int64_t, int64_t, int64_t, int64_t, int, int, float,
    bool, hipStream_t);
void framestack_gather_shift_launch(const unsigned char*, const int64_t*,
                                    const int*, unsigned char*,
                                    unsigned char*, int64_t, int64_t, int,
                                    int, int, bool, hipStream_t);
void framestack_gather_nstep_shift_launch(
    const unsigned char*, const int64_t*, const int64_t*, const float*,
    const float*, const int64_t*, const int*, unsigned char*,
    unsigned char*, float*, float*, int64_t*, int64_t, int64_t, int64_t,
    int, int, int, int, float, bool, hipStream_t);
void framestack_vec_append_launch(
    unsigned char*, float*, float*, int64_t*, int64_t*, int64_t*,
    const unsigned char*, const unsigned char*, const float*, const float*,
    const float*, const float*, int64_t*, int64_t*, float*, int64_t, int64_t,
    int64_t, int, int, bool, hipStream_t);
void pixelcatch_step_launch(int32_t*, int64_t*, const int64_t*,
                            unsigned char*, unsigned char*, float*, float*,
                            int32_t*, unsigned char*, int64_t*, float*,
                            float*, int64_t, uint64_t, int, int, int, bool,
                            bool, hipStream_t);
void pixelcatch_reset_launch(int32_t*, int64_t*, const unsigned char*,
                             unsigned char*, int64_t, uint64_t, int, bool,
                             hipStream_t);
void pg_head_fwd_launch(const void*, const int64_t*, float*, float*,
                        int64_t, int, hipStream_t);
void pg_head_bwd_launch(const void*, const int64_t*, const float*,
                        const float*, void*, int64_t, int, hipStream_t);
void conv1_wrw_launch(const void*, const unsigned char*, float*, float*,
                      float*, int64_t, float, hipStream_t);
void mfma_probe_launch(const void*, const void*, float*, hipStream_t);
void tr16_probe_launch(float*, int, hipStream_t);
void fwd_bfrag_probe_launch(float*, int, hipStream_t);
void tr16_diag_launch(float*, int, hipStream_t);
void conv1_fwd_launch(const unsigned char*, const void*, const float*,
                      void*, int64_t, float, hipStream_t);
void conv1_fwd_relu_launch(const unsigned char*, const void*, const float*,
                           void*, unsigned int*, int64_t, float,
                           hipStream_t);
void conv1_wrw_masked_launch(const void*, const unsigned int*,
                             const unsigned char*, float*, float*, float*,
                             int64_t, float, hipStream_t);
void bias_relu_launch(void*, const float*, int64_t, int, hipStream_t);
int64_t bias_relu_bwd_blocks(int64_t, int);
void bias_relu_bwd_launch(const void*, const void*, void*, float*, float*,
                          int64_t, int, hipStream_t);
int64_t bias_relu_flat_blocks(int64_t);
void bias_relu_flat_launch(const void*, const float*, void*, int64_t, int,
                           int, hipStream_t);
void bias_relu_flat_bwd_launch(const void*, const void*, void*, float*,
                               float*, int64_t, int, int, hipStream_t);

void noisy_linear_fwd_launch(const void*, const float*, const float*,
                             const float*, const float*, const float*,
                             const float*, void*, float*, int, int, int, int,
                             int, bool, hipStream_t);
void noisy_linear_bwd_input_launch(const void*, const float*, const float*,
                                   const float*, const float*, void*, float*,
                                   int, int, int, int, int, bool,
                                   hipStream_t);
void noisy_linear_bwd_weight_launch(const void*, const void*, const float*,
                                    const float*, float*, float*, float*,
                                    float*, int, int, int, bool, hipStream_t);
void factorised_noise_launch(float*, int64_t, uint64_t, uint64_t,
                             hipStream_t);
int noisy_linear_slices(int64_t, int64_t, int64_t, int*);

namespace {

void check_f32_cuda(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a CUDA tensor");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// Every further tensor argument of an op: on `ref`'s device, of dtype
// `dt`, contiguous and holding exactly `numel` elements. Runs before
// the launch, so a kernel never indexes a short or foreign buffer.
void check_arg(const Tensor& t, const Tensor& ref, at::ScalarType dt,
               int64_t numel, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), name,
              " must be a CUDA tensor on the first argument's device");
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() == numel, name, " must hold ", numel,
              " elements, got ", t.numel());
}

// [rows, cols] float32 first argument of the scans and heads
void check_f32_2d(const Tensor& t, const char* name) {
  check_f32_cuda(t, name);
  TORCH_CHECK(t.dim() == 2, name, " must be 2-D");
}

// tree [2 * capacity] float32 with capacity == 2^depth
void check_tree(const Tensor& tree, int64_t capacity, int64_t depth) {
  check_f32_cuda(tree, "tree");
  TORCH_CHECK(depth >= 1 && depth < 62 &&
                  capacity == ((int64_t)1 << depth),
              "capacity must be 2^depth with depth >= 1");
  TORCH_CHECK(tree.numel() == 2 * capacity,
              "tree must hold 2 * capacity elements");
  // the sampling walk loads the two children of a node as one float2
  TORCH_CHECK((uintptr_t)tree.data_ptr() % 8 == 0,
              "tree must be 8-byte aligned");
}

hipStream_t current_stream() {
  return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}

// ------------------------------------------------------------------
// sum-tree
// ------------------------------------------------------------------
void sumtree_update(Tensor tree, Tensor idx, Tensor w, int64_t capacity,
                    int64_t depth) {
  check_tree(tree, capacity, depth);
  check_arg(idx, tree, at::kLong, idx.numel(), "idx");
  check_arg(w, tree, at::kFloat, idx.numel(), "w");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(tree.device());
  sumtree_update_launch(tree.data_ptr<float>(), idx.data_ptr<int64_t>(),
                        w.data_ptr<float>(), idx.numel(), capacity,
                        (int)depth, current_stream());
}

void sumtree_build(Tensor tree, int64_t capacity) {
  check_f32_cuda(tree, "tree");
  TORCH_CHECK(capacity >= 2 && (capacity & (capacity - 1)) == 0 &&
                  tree.numel() == 2 * capacity,
              "tree must hold 2 * capacity elements, capacity a power of "
              "two >= 2");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(tree.device());
  sumtree_build_launch(tree.data_ptr<float>(), capacity, current_stream());
}

Tensor sumtree_sample(Tensor tree, Tensor u, int64_t capacity, int64_t depth,
                      int64_t size) {
  check_tree(tree, capacity, depth);
  check_arg(u, tree, at::kFloat, u.numel(), "u");
  TORCH_CHECK(size >= 1 && size <= capacity,
              "size must be in [1, capacity]");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(tree.device());
  Tensor out = at::empty({u.numel()}, u.options().dtype(at::kLong));
  sumtree_sample_launch(tree.data_ptr<float>(), u.data_ptr<float>(),
                        out.data_ptr<int64_t>(), u.numel(), capacity,
                        (int)depth, size, current_stream());
  return out;
}

// ------------------------------------------------------------------
// scans
// ------------------------------------------------------------------
Tensor discounted_returns(Tensor rew, Tensor nd, Tensor bootstrap,
                          double gamma) {
  check_f32_2d(rew, "rewards");
  int64_t T = rew.size(0), B = rew.size(1);
  check_arg(nd, rew, at::kFloat, T * B, "non-terminal mask");
  check_arg(bootstrap, rew, at::kFloat, B, "bootstrap");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(rew.device());
  Tensor out = at::empty_like(rew);
  discounted_returns_launch(rew.data_ptr<float>(), nd.data_ptr<float>(),
                            bootstrap.data_ptr<float>(),
                            out.data_ptr<float>(), T, B, (float)gamma,
                            current_stream());
  return out;
}

Tensor gae(Tensor rew, Tensor val, Tensor next_val, Tensor nd, double gamma,
           double lam) {
  check_f32_2d(rew, "rewards");
  int64_t T = rew.size(0), B = rew.size(1);
  check_arg(val, rew, at::kFloat, T * B, "values");
  check_arg(next_val, rew, at::kFloat, T * B, "next_values");
  check_arg(nd, rew, at::kFloat, T * B, "non-terminal mask");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(rew.device());
  Tensor out = at::empty_like(rew);
  gae_launch(rew.data_ptr<float>(), val.data_ptr<float>(),
             next_val.data_ptr<float>(), nd.data_ptr<float>(),
             out.data_ptr<float>(), T, B, (float)gamma, (float)lam,
             current_stream());
  return out;
}

std::vector<Tensor> vtrace(Tensor blp, Tensor tlp, Tensor rew, Tensor val,
                           Tensor bootstrap, Tensor nd, double gamma,
                           double rho_clip, double c_clip,
                           double pg_rho_clip) {
  check_f32_2d(rew, "rewards");
  int64_t T = rew.size(0), B = rew.size(1);
  check_arg(blp, rew, at::kFloat, T * B, "behavior_log_probs");
  check_arg(tlp, rew, at::kFloat, T * B, "target_log_probs");
  check_arg(val, rew, at::kFloat, T * B, "values");
  check_arg(nd, rew, at::kFloat, T * B, "non-terminal mask");
  check_arg(bootstrap, rew, at::kFloat, B, "bootstrap_value");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(rew.device());
  Tensor vs = at::empty_like(rew);
  Tensor pg_adv = at::empty_like(rew);
  vtrace_launch(blp.data_ptr<float>(), tlp.data_ptr<float>(),
                rew.data_ptr<float>(), val.data_ptr<float>(),
                bootstrap.data_ptr<float>(), nd.data_ptr<float>(),
                vs.data_ptr<float>(), pg_adv.data_ptr<float>(), T, B,
                (float)gamma, (float)rho_clip, (float)c_clip,
                (float)pg_rho_clip, current_stream());
  return {vs, pg_adv};
}

std::vector<Tensor> vtrace_bt(Tensor blp, Tensor tlp, Tensor rew,
                              Tensor val, Tensor bootstrap, Tensor nd,
                              double gamma, double rho_clip,
                              double c_clip, double pg_rho_clip) {
  check_f32_2d(rew, "rewards");
  int64_t B = rew.size(0), T = rew.size(1);
  check_arg(blp, rew, at::kFloat, T * B, "behavior_log_probs");
  check_arg(tlp, rew, at::kFloat, T * B, "target_log_probs");
  check_arg(val, rew, at::kFloat, T * B, "values");
  check_arg(nd, rew, at::kFloat, T * B, "non-terminal mask");
  check_arg(bootstrap, rew, at::kFloat, B, "bootstrap_value");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(rew.device());
  Tensor vs = at::empty_like(rew);
  Tensor pg_adv = at::empty_like(rew);
  vtrace_bt_launch(blp.data_ptr<float>(), tlp.data_ptr<float>(),
                   rew.data_ptr<float>(), val.data_ptr<float>(),
                   bootstrap.data_ptr<float>(), nd.data_ptr<float>(),
                   vs.data_ptr<float>(), pg_adv.data_ptr<float>(), T, B,
                   (float)gamma, (float)rho_clip, (float)c_clip,
                   (float)pg_rho_clip, current_stream());
  return {vs, pg_adv};
}

Tensor nstep_returns(Tensor rew, Tensor alive, double gamma, int64_t n) {
  check_f32_2d(rew, "rewards");
  int64_t T = rew.size(0), B = rew.size(1);
  check_arg(alive, rew, at::kFloat, T * B, "alive");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(rew.device());
  Tensor out = at::empty_like(rew);
  nstep_returns_launch(rew.data_ptr<float>(), alive.data_ptr<float>(),
                       out.data_ptr<float>(), T, B, (float)gamma, (int)n,
                       current_stream());
  return out;
}

// ------------------------------------------------------------------
// categorical projection
// ------------------------------------------------------------------
Tensor categorical_projection(Tensor next_dist, Tensor rew, Tensor nd,
                              double gamma, double v_min, double v_max) {
  check_f32_2d(next_dist, "next_dist");
  int64_t B = next_dist.size(0), A = next_dist.size(1);
  TORCH_CHECK(A >= 2 && A <= 256,
              "categorical projection supports 2 to 256 atoms");
  check_arg(rew, next_dist, at::kFloat, B, "rewards");
  check_arg(nd, next_dist, at::kFloat, B, "non-terminal mask");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(next_dist.device());
  Tensor out = at::empty_like(next_dist);
  categorical_projection_launch(next_dist.data_ptr<float>(),
                                rew.data_ptr<float>(), nd.data_ptr<float>(),
                                out.data_ptr<float>(), B, A, (float)gamma,
                                (float)v_min, (float)v_max,
                                current_stream());
  return out;
}

// ------------------------------------------------------------------
// NoisyLinear (semantics: machin_amd.ops.noisy_linear)
// ------------------------------------------------------------------
// x or dy [B, cols] fp32 / bf16; mu, sigma [O, I]; eps_in [I], eps_out [O]
void check_noisy(const Tensor& a, int64_t cols, const Tensor& mu,
                 const Tensor& sigma, const Tensor& eps_in,
                 const Tensor& eps_out, const char* name) {
  TORCH_CHECK(a.is_cuda() && a.is_contiguous() && a.dim() == 2, name,
              " must be a contiguous 2-D CUDA tensor");
  TORCH_CHECK(a.scalar_type() == at::kFloat ||
                  a.scalar_type() == at::kBFloat16,
              name, " must be float32 or bfloat16");
  TORCH_CHECK(mu.dim() == 2 && mu.size(0) >= 1 && mu.size(1) >= 1,
              "weight_mu must be [O, I]");
  const int64_t O = mu.size(0), I = mu.size(1);
  TORCH_CHECK(O * I < ((int64_t)1 << 31), "O * I must be below 2^31");
  TORCH_CHECK(a.size(0) >= 1 && a.size(0) <= 65535 * 32,
              "batch must be in [1, 2097120]");
  TORCH_CHECK(a.size(1) == cols, name, " has the wrong row length");
  check_arg(mu, a, at::kFloat, O * I, "weight_mu");
  check_arg(sigma, a, at::kFloat, O * I, "weight_sigma");
  check_arg(eps_in, a, at::kFloat, I, "eps_in");
  check_arg(eps_out, a, at::kFloat, O, "eps_out");
}

Tensor noisy_linear_fwd(Tensor x, Tensor mu, Tensor sigma, Tensor bias_mu,
                        Tensor bias_sigma, Tensor eps_in, Tensor eps_out) {
  TORCH_CHECK(mu.dim() == 2, "weight_mu must be [O, I]");
  const int64_t O = mu.size(0), I = mu.size(1);
  check_noisy(x, I, mu, sigma, eps_in, eps_out, "x");
  check_arg(bias_mu, x, at::kFloat, O, "bias_mu");
  check_arg(bias_sigma, x, at::kFloat, O, "bias_sigma");
  const int64_t B = x.size(0);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({B, O}, x.options());
  int cps = 1;
  const int S = noisy_linear_slices(B, O, I, &cps);
  Tensor part;
  float* part_ptr = nullptr;
  if (S > 1) {
    part = at::empty({S, B, O}, x.options().dtype(at::kFloat));
    part_ptr = part.data_ptr<float>();
  }
  noisy_linear_fwd_launch(
      x.data_ptr(), mu.data_ptr<float>(), sigma.data_ptr<float>(),
      bias_mu.data_ptr<float>(), bias_sigma.data_ptr<float>(),
      eps_in.data_ptr<float>(), eps_out.data_ptr<float>(), y.data_ptr(),
      part_ptr, (int)B, (int)I, (int)O, cps, S,
      x.scalar_type() == at::kBFloat16, current_stream());
  return y;
}

Tensor noisy_linear_bwd_input(Tensor dy, Tensor mu, Tensor sigma,
                              Tensor eps_in, Tensor eps_out) {
  TORCH_CHECK(mu.dim() == 2, "weight_mu must be [O, I]");
  const int64_t O = mu.size(0), I = mu.size(1);
  check_noisy(dy, O, mu, sigma, eps_in, eps_out, "dy");
  const int64_t B = dy.size(0);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dy.device());
  Tensor dx = at::empty({B, I}, dy.options());
  int cps = 1;
  const int S = noisy_linear_slices(B, I, O, &cps);
  Tensor part;
  float* part_ptr = nullptr;
  if (S > 1) {
    part = at::empty({S, B, I}, dy.options().dtype(at::kFloat));
    part_ptr = part.data_ptr<float>();
  }
  noisy_linear_bwd_input_launch(
      dy.data_ptr(), mu.data_ptr<float>(), sigma.data_ptr<float>(),
      eps_in.data_ptr<float>(), eps_out.data_ptr<float>(), dx.data_ptr(),
      part_ptr, (int)B, (int)I, (int)O, cps, S,
      dy.scalar_type() == at::kBFloat16, current_stream());
  return dx;
}

// Returns {dmu [O, I], dsigma [O, I], dbias_mu [O], dbias_sigma [O]}.
std::vector<Tensor> noisy_linear_bwd_weight(Tensor dy, Tensor x,
                                            Tensor eps_in, Tensor eps_out) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() == 2,
              "dy must be a contiguous 2-D CUDA tensor");
  TORCH_CHECK(dy.scalar_type() == at::kFloat ||
                  dy.scalar_type() == at::kBFloat16,
              "dy must be float32 or bfloat16");
  TORCH_CHECK(x.dim() == 2 && x.size(0) == dy.size(0),
              "x must be [B, I] with dy's batch");
  const int64_t B = dy.size(0), O = dy.size(1), I = x.size(1);
  TORCH_CHECK(B >= 1 && B < ((int64_t)1 << 31) && O >= 1 && I >= 1 &&
                  O * I < ((int64_t)1 << 31) && O <= 65535 * 32,
              "need B, I, O >= 1, O * I < 2^31 and O <= 2097120");
  check_arg(x, dy, dy.scalar_type(), B * I, "x");
  check_arg(eps_in, dy, at::kFloat, I, "eps_in");
  check_arg(eps_out, dy, at::kFloat, O, "eps_out");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dy.device());
  const auto f32 = dy.options().dtype(at::kFloat);
  Tensor dmu = at::empty({O, I}, f32);
  Tensor dsigma = at::empty({O, I}, f32);
  Tensor dbias_mu = at::empty({O}, f32);
  Tensor dbias_sigma = at::empty({O}, f32);
  noisy_linear_bwd_weight_launch(
      dy.data_ptr(), x.data_ptr(), eps_in.data_ptr<float>(),
      eps_out.data_ptr<float>(), dmu.data_ptr<float>(),
      dsigma.data_ptr<float>(), dbias_mu.data_ptr<float>(),
      dbias_sigma.data_ptr<float>(), (int)B, (int)I, (int)O,
      dy.scalar_type() == at::kBFloat16, current_stream());
  return {dmu, dsigma, dbias_mu, dbias_sigma};
}

// {slices S, steps per slice} of the forward / dx reduction for a
// [B, N] output reduced over K: what the two launchers above use
std::vector<int64_t> noisy_linear_slices_py(int64_t B, int64_t N,
                                            int64_t K) {
  TORCH_CHECK(B >= 1 && N >= 1 && K >= 1, "need B, N, K >= 1");
  int cps = 1;
  const int S = noisy_linear_slices(B, N, K, &cps);
  return {S, cps};
}

void factorised_noise_(Tensor buf, int64_t seed, int64_t offset) {
  check_f32_cuda(buf, "buf");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(buf.device());
  factorised_noise_launch(buf.data_ptr<float>(), buf.numel(), (uint64_t)seed,
                          (uint64_t)offset, current_stream());
}

// ------------------------------------------------------------------
// fused C51 loss head (semantics: machin_amd.ops.c51_loss)
// ------------------------------------------------------------------
void check_c51_dist(const Tensor& t, const Tensor& like, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 3, name,
              " must be a contiguous [B, A, N] CUDA tensor");
  TORCH_CHECK(t.scalar_type() == like.scalar_type() &&
                  t.sizes() == like.sizes() && t.device() == like.device(),
              name, " must match dist in dtype, shape and device");
}

void check_c51_rows(const Tensor& t, const Tensor& dist, at::ScalarType dt,
                    const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == dist.device() &&
                  t.scalar_type() == dt && t.is_contiguous() &&
                  t.dim() == 1 && t.size(0) == dist.size(0),
              name, " must be a contiguous [B] ", dt,
              " tensor on dist's device");
}

// Returns {loss [B], proj [B, N], best [B] int64, lse [B], S [B]}.
// An undefined `discount` means the scalar one for every row.
std::vector<Tensor> c51_loss_fwd(Tensor dist, Tensor action,
                                 Tensor next_online, Tensor next_target,
                                 Tensor reward, Tensor terminal,
                                 c10::optional<Tensor> discount,
                                 double discount_scalar, double v_min,
                                 double v_max, bool from_logits) {
  TORCH_CHECK(dist.scalar_type() == at::kFloat ||
                  dist.scalar_type() == at::kBFloat16,
              "dist must be float32 or bfloat16");
  check_c51_dist(dist, dist, "dist");
  check_c51_dist(next_online, dist, "next_online");
  check_c51_dist(next_target, dist, "next_target");
  const int64_t B = dist.size(0), A = dist.size(1), N = dist.size(2);
  TORCH_CHECK(N >= 2 && N <= 256, "atoms must be in [2, 256]");
  TORCH_CHECK(A >= 1 && A <= 64, "actions must be in [1, 64]");
  TORCH_CHECK(v_min < v_max, "v_min must be below v_max");
  check_c51_rows(action, dist, at::kLong, "action");
  check_c51_rows(reward, dist, at::kFloat, "reward");
  check_c51_rows(terminal, dist, at::kFloat, "terminal");
  const float* discount_ptr = nullptr;
  if (discount.has_value() && discount->defined()) {
    check_c51_rows(*discount, dist, at::kFloat, "discount");
    discount_ptr = discount->data_ptr<float>();
  }
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dist.device());
  const auto f32 = dist.options().dtype(at::kFloat);
  Tensor loss = at::empty({B}, f32);
  Tensor proj = at::empty({B, N}, f32);
  Tensor best = at::empty({B}, dist.options().dtype(at::kLong));
  Tensor lse = at::empty({B}, f32);
  Tensor s_sum = at::empty({B}, f32);
  c51_loss_fwd_launch(
      dist.data_ptr(), action.data_ptr<int64_t>(), next_online.data_ptr(),
      next_target.data_ptr(), reward.data_ptr<float>(),
      terminal.data_ptr<float>(), discount_ptr, (float)discount_scalar,
      loss.data_ptr<float>(), proj.data_ptr<float>(),
      best.data_ptr<int64_t>(), lse.data_ptr<float>(),
      s_sum.data_ptr<float>(), B, (int)A, (int)N, (float)v_min,
      (float)v_max, dist.scalar_type() == at::kBFloat16, from_logits,
      current_stream());
  return {loss, proj, best, lse, s_sum};
}

// grad_dist in dist's dtype, every element written.
Tensor c51_loss_bwd(Tensor dist, Tensor action, Tensor proj, Tensor lse,
                    Tensor s_sum, Tensor g, bool from_logits) {
  TORCH_CHECK(dist.scalar_type() == at::kFloat ||
                  dist.scalar_type() == at::kBFloat16,
              "dist must be float32 or bfloat16");
  check_c51_dist(dist, dist, "dist");
  const int64_t B = dist.size(0), A = dist.size(1), N = dist.size(2);
  TORCH_CHECK(N >= 2 && N <= 256, "atoms must be in [2, 256]");
  TORCH_CHECK(A >= 1 && A <= 64, "actions must be in [1, 64]");
  check_c51_rows(action, dist, at::kLong, "action");
  check_c51_rows(lse, dist, at::kFloat, "lse");
  check_c51_rows(s_sum, dist, at::kFloat, "S");
  check_c51_rows(g, dist, at::kFloat, "g");
  TORCH_CHECK(proj.is_cuda() && proj.device() == dist.device() &&
                  proj.scalar_type() == at::kFloat && proj.is_contiguous() &&
                  proj.dim() == 2 && proj.size(0) == B && proj.size(1) == N,
              "proj must be a contiguous [B, N] float32 tensor on dist's "
              "device");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dist.device());
  Tensor grad = at::empty_like(dist);
  c51_loss_bwd_launch(dist.data_ptr(), action.data_ptr<int64_t>(),
                      proj.data_ptr<float>(), lse.data_ptr<float>(),
                      s_sum.data_ptr<float>(), g.data_ptr<float>(),
                      grad.data_ptr(), B, (int)A, (int)N,
                      dist.scalar_type() == at::kBFloat16, from_logits,
                      current_stream());
  return grad;
}

// ------------------------------------------------------------------
// multi-tensor polyak
// ------------------------------------------------------------------
void multi_tensor_polyak(std::vector<Tensor> targets,
                         std::vector<Tensor> sources, double tau) {
  TORCH_CHECK(targets.size() == sources.size(), "list size mismatch");
  if (targets.empty()) return;
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(targets[0].device());
  int64_t n = (int64_t)targets.size();
  // host-side table: [tgt_ptr, src_ptr] pairs then exclusive prefix
  Tensor table = at::empty({n * 2 + n + 1},
                           at::TensorOptions().dtype(at::kLong));
  int64_t* h = table.data_ptr<int64_t>();
  int64_t total = 0;
  for (int64_t i = 0; i < n; ++i) {
    check_f32_cuda(targets[i], "target");
    check_f32_cuda(sources[i], "source");
    TORCH_CHECK(targets[i].numel() == sources[i].numel(), "numel mismatch");
    h[2 * i] = (int64_t)targets[i].data_ptr<float>();
    h[2 * i + 1] = (int64_t)sources[i].data_ptr<float>();
    h[2 * n + i] = total;
    total += targets[i].numel();
  }
  h[2 * n + n] = total;
  Tensor dev_table = table.to(targets[0].device(), /*non_blocking=*/true);
  int64_t* d = dev_table.data_ptr<int64_t>();
  multi_tensor_polyak_launch((void*)d, d + 2 * n, n, total, (float)tau,
                             current_stream());
}

// Cached variant: the python layer builds the device table ONCE per
// (targets, sources) pair; each call is then a single kernel launch
// with zero host-side setup (the v1 per-call table build made the
// fused kernel 6x slower than torch _foreach on small nets,
// profiles/kernel_bench_r01.json).
void multi_tensor_polyak_cached(Tensor dev_table, int64_t n_tensors,
                                int64_t total, double tau) {
  TORCH_CHECK(dev_table.is_cuda() &&
                  dev_table.scalar_type() == at::kLong &&
                  dev_table.is_contiguous(),
              "dev_table must be contiguous int64 CUDA");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(
      dev_table.device());
  int64_t* d = dev_table.data_ptr<int64_t>();
  multi_tensor_polyak_launch((void*)d, d + 2 * n_tensors, n_tensors, total,
                             (float)tau, current_stream());
}

// Cached-plan fused clip+RMSprop: dev_table = [p,g,sq]*n ptrs then
// the n+1 prefix; norm_buf = one fp32 scratch.
void fused_rmsprop_cached(Tensor dev_table, int64_t n_tensors,
                          int64_t total, Tensor norm_buf,
                          double max_norm, double lr, double alpha,
                          double eps) {
  TORCH_CHECK(dev_table.is_cuda() &&
                  dev_table.scalar_type() == at::kLong &&
                  dev_table.is_contiguous(),
              "dev_table must be contiguous int64 CUDA");
  check_f32_cuda(norm_buf, "norm_buf");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(
      dev_table.device());
  int64_t* d = dev_table.data_ptr<int64_t>();
  fused_rmsprop_launch((void*)d, d + 3 * n_tensors, n_tensors, total,
                       norm_buf.data_ptr<float>(), (float)max_norm,
                       (float)lr, (float)alpha, (float)eps,
                       current_stream());
}

// ------------------------------------------------------------------
// distributions
// ------------------------------------------------------------------
std::vector<Tensor> gaussian_sample_logprob(Tensor mu, Tensor log_std,
                                            int64_t seed, int64_t offset,
                                            bool tanh_squash,
                                            double epsilon) {
  check_f32_2d(mu, "mu");
  int64_t B = mu.size(0), D = mu.size(1);
  check_arg(log_std, mu, at::kFloat, B * D, "log_std");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(mu.device());
  Tensor act = at::empty_like(mu);
  Tensor logp = at::empty({B, 1}, mu.options());
  gaussian_sample_logprob_launch(
      mu.data_ptr<float>(), log_std.data_ptr<float>(), act.data_ptr<float>(),
      logp.data_ptr<float>(), B, D, (uint64_t)seed, (uint64_t)offset,
      tanh_squash ? 1 : 0, (float)epsilon, current_stream());
  return {act, logp};
}

Tensor gaussian_logprob(Tensor mu, Tensor log_std, Tensor act,
                        bool tanh_squash, double epsilon) {
  check_f32_2d(mu, "mu");
  int64_t B = mu.size(0), D = mu.size(1);
  check_arg(log_std, mu, at::kFloat, B * D, "log_std");
  check_arg(act, mu, at::kFloat, B * D, "act");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(mu.device());
  Tensor logp = at::empty({B, 1}, mu.options());
  gaussian_logprob_launch(mu.data_ptr<float>(), log_std.data_ptr<float>(),
                          act.data_ptr<float>(), logp.data_ptr<float>(), B,
                          D, tanh_squash ? 1 : 0, (float)epsilon,
                          current_stream());
  return logp;
}

void normal_noise_(Tensor x, double mean, double std, int64_t seed,
                   int64_t offset, bool add) {
  check_f32_cuda(x, "x");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  normal_noise_launch(x.data_ptr<float>(), x.numel(), (float)mean,
                      (float)std, (uint64_t)seed, (uint64_t)offset,
                      add ? 1 : 0, current_stream());
}

void ou_update_(Tensor x, double mu, double theta, double sigma, double dt,
                int64_t seed, int64_t offset) {
  check_f32_cuda(x, "x");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  ou_update_launch(x.data_ptr<float>(), x.numel(), (float)mu, (float)theta,
                   (float)sigma, (float)dt, (uint64_t)seed,
                   (uint64_t)offset, current_stream());
}

std::vector<Tensor> pg_head_fwd(Tensor logits, Tensor actions) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16 &&
                  logits.is_contiguous(),
              "logits must be contiguous bf16 CUDA [N, A]");
  TORCH_CHECK(logits.dim() == 2, "logits must be 2-D");
  int64_t N = logits.size(0), A = logits.size(1);
  TORCH_CHECK(A >= 1 && A <= 32, "pg_head supports 1 to 32 actions");
  check_arg(actions, logits, at::kLong, N, "actions");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(logits.device());
  Tensor tl = at::empty({N}, logits.options().dtype(at::kFloat));
  Tensor ent = at::empty({N}, logits.options().dtype(at::kFloat));
  pg_head_fwd_launch(logits.data_ptr(), actions.data_ptr<int64_t>(),
                     tl.data_ptr<float>(), ent.data_ptr<float>(), N,
                     (int)A, current_stream());
  return {tl, ent};
}

Tensor pg_head_bwd(Tensor logits, Tensor actions, Tensor g_taken,
                   Tensor g_ent) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16 &&
                  logits.is_contiguous() && logits.dim() == 2,
              "logits must be contiguous bf16 CUDA [N, A]");
  int64_t N = logits.size(0), A = logits.size(1);
  TORCH_CHECK(A >= 1 && A <= 32, "pg_head supports 1 to 32 actions");
  check_arg(actions, logits, at::kLong, N, "actions");
  check_arg(g_taken, logits, at::kFloat, N, "g_taken");
  check_arg(g_ent, logits, at::kFloat, N, "g_ent");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(logits.device());
  Tensor d = at::empty_like(logits);
  pg_head_bwd_launch(logits.data_ptr(), actions.data_ptr<int64_t>(),
                     g_taken.data_ptr<float>(), g_ent.data_ptr<float>(),
                     d.data_ptr(), N, (int)A, current_stream());
  return d;
}

Tensor u8_to_bf16_scale(Tensor in, double scale) {
  TORCH_CHECK(in.is_cuda() && in.scalar_type() == at::kByte &&
                  in.is_contiguous(),
              "input must be contiguous uint8 CUDA");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in.device());
  Tensor out = at::empty_like(in, in.options().dtype(at::kBFloat16));
  u8_to_bf16_scale_launch(in.data_ptr<unsigned char>(), out.data_ptr(),
                          in.numel(), (float)scale, current_stream());
  return out;
}

// frame-deduplicated replay: rebuild (state, next_state) stacks
// [B, k, H, W] from a ring of u8 planes [P, H, W]; window plane j of
// sample b is ring slot (base[b] + j) mod P. The kernel reduces base
// modulo P itself, so values are never inspected on the host.
//
// shift (may be null): int32 [B, 4] = (dy_state, dx_state, dy_next,
// dx_next), the random-shift augmentation fused into the gather; null
// launches exactly the un-shifted kernels.
static void framestack_check_shift(const Tensor& shift,
                                   const Tensor& planes, int64_t B) {
  TORCH_CHECK(shift.is_cuda() && shift.device() == planes.device(),
              "shift must be on the device of planes");
  TORCH_CHECK(shift.scalar_type() == at::kInt, "shift must be int32");
  TORCH_CHECK(shift.dim() == 2 && shift.size(0) == B && shift.size(1) == 4,
              "shift must be [B, 4]");
  TORCH_CHECK(shift.is_contiguous(), "shift must be contiguous");
  TORCH_CHECK(planes.size(1) * planes.size(2) < (int64_t(1) << 30),
              "shifted gather needs H * W < 2^30");
}

static std::vector<Tensor> framestack_gather_impl(const Tensor& planes,
                                                  const Tensor& base,
                                                  int64_t k,
                                                  bool channels_last,
                                                  const Tensor* shift) {
  TORCH_CHECK(planes.is_cuda() && planes.scalar_type() == at::kByte &&
                  planes.is_contiguous(),
              "planes must be contiguous uint8 CUDA");
  TORCH_CHECK(planes.dim() == 3, "planes must be [P, H, W]");
  TORCH_CHECK(base.is_cuda() && base.scalar_type() == at::kLong &&
                  base.is_contiguous() && base.dim() == 1,
              "base must be contiguous 1-D int64 CUDA");
  TORCH_CHECK(base.device() == planes.device(),
              "planes and base must be on the same device");
  TORCH_CHECK(k >= 1 && k <= 8, "k must be in [1, 8]");
  const int64_t P = planes.size(0), H = planes.size(1), W = planes.size(2);
  TORCH_CHECK(P >= k + 1, "ring needs at least k+1 planes");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(planes.device());
  const int64_t B = base.numel();
  if (shift != nullptr) framestack_check_shift(*shift, planes, B);
  const auto fmt = channels_last ? at::MemoryFormat::ChannelsLast
                                 : at::MemoryFormat::Contiguous;
  Tensor state = at::empty({B, k, H, W}, planes.options(), fmt);
  Tensor next = at::empty({B, k, H, W}, planes.options(), fmt);
  if (shift != nullptr) {
    framestack_gather_shift_launch(
        planes.data_ptr<unsigned char>(), base.data_ptr<int64_t>(),
        shift->data_ptr<int>(), state.data_ptr<unsigned char>(),
        next.data_ptr<unsigned char>(), B, P, (int)H, (int)W, (int)k,
        channels_last, current_stream());
    return {state, next};
  }
  framestack_gather_launch(planes.data_ptr<unsigned char>(),
                           base.data_ptr<int64_t>(),
                           state.data_ptr<unsigned char>(),
                           next.data_ptr<unsigned char>(), B, P, H * W,
                           (int)k, channels_last, current_stream());
  return {state, next};
}

std::vector<Tensor> framestack_gather(Tensor planes, Tensor base, int64_t k,
                                      bool channels_last) {
  return framestack_gather_impl(planes, base, k, channels_last, nullptr);
}

std::vector<Tensor> framestack_gather_shift(Tensor planes, Tensor base,
                                            int64_t k, bool channels_last,
                                            Tensor shift) {
  return framestack_gather_impl(planes, base, k, channels_last, &shift);
}

// n-step variant: the kernel indexes the whole transition-ring columns
// base/left/reward/terminal [T] with the sampled positions pos [B] and
// returns (state, next_state, reward_n, terminal_n, steps); semantics
// in framestack.hip. All indices are reduced or clamped in the kernel.
static std::vector<Tensor> framestack_gather_nstep_impl(
    const Tensor& planes, const Tensor& base, const Tensor& left,
    const Tensor& reward, const Tensor& terminal, const Tensor& pos,
    int64_t k, int64_t n, double gamma, bool channels_last,
    const Tensor* shift) {
  TORCH_CHECK(planes.is_cuda() && planes.scalar_type() == at::kByte &&
                  planes.is_contiguous(),
              "planes must be contiguous uint8 CUDA");
  TORCH_CHECK(planes.dim() == 3, "planes must be [P, H, W]");
  TORCH_CHECK(k >= 1 && k <= 8, "k must be in [1, 8]");
  TORCH_CHECK(n >= 1 && n <= 16, "n must be in [1, 16]");
  const int64_t P = planes.size(0), H = planes.size(1), W = planes.size(2);
  TORCH_CHECK(P >= k + n, "ring needs at least k+n planes");
  TORCH_CHECK(H * W > 0, "planes must not be empty");
  const int64_t T = base.numel();
  TORCH_CHECK(T >= 1, "transition ring needs at least one row");
  for (const Tensor* c : {&base, &left, &pos}) {
    TORCH_CHECK(c->is_cuda() && c->scalar_type() == at::kLong &&
                    c->is_contiguous() && c->dim() == 1,
                "base, left and pos must be contiguous 1-D int64 CUDA");
  }
  for (const Tensor* c : {&reward, &terminal}) {
    TORCH_CHECK(c->is_cuda() && c->scalar_type() == at::kFloat &&
                    c->is_contiguous() && c->dim() == 1,
                "reward and terminal must be contiguous 1-D float32 CUDA");
  }
  for (const Tensor* c : {&base, &left, &reward, &terminal, &pos}) {
    TORCH_CHECK(c->device() == planes.device(),
                "all tensors must be on the same device");
  }
  TORCH_CHECK(left.numel() == T && reward.numel() == T &&
                  terminal.numel() == T,
              "base, left, reward and terminal must have the same length");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(planes.device());
  const int64_t B = pos.numel();
  if (shift != nullptr) framestack_check_shift(*shift, planes, B);
  const auto fmt = channels_last ? at::MemoryFormat::ChannelsLast
                                 : at::MemoryFormat::Contiguous;
  Tensor state = at::empty({B, k, H, W}, planes.options(), fmt);
  Tensor next = at::empty({B, k, H, W}, planes.options(), fmt);
  Tensor reward_n = at::empty({B}, reward.options());
  Tensor terminal_n = at::empty({B}, reward.options());
  Tensor steps = at::empty({B}, pos.options());
  if (shift != nullptr) {
    framestack_gather_nstep_shift_launch(
        planes.data_ptr<unsigned char>(), base.data_ptr<int64_t>(),
        left.data_ptr<int64_t>(), reward.data_ptr<float>(),
        terminal.data_ptr<float>(), pos.data_ptr<int64_t>(),
        shift->data_ptr<int>(), state.data_ptr<unsigned char>(),
        next.data_ptr<unsigned char>(), reward_n.data_ptr<float>(),
        terminal_n.data_ptr<float>(), steps.data_ptr<int64_t>(), B, P, T,
        (int)H, (int)W, (int)k, (int)n, (float)gamma, channels_last,
        current_stream());
    return {state, next, reward_n, terminal_n, steps};
  }
  framestack_gather_nstep_launch(
      planes.data_ptr<unsigned char>(), base.data_ptr<int64_t>(),
      left.data_ptr<int64_t>(), reward.data_ptr<float>(),
      terminal.data_ptr<float>(), pos.data_ptr<int64_t>(),
      state.data_ptr<unsigned char>(), next.data_ptr<unsigned char>(),
      reward_n.data_ptr<float>(), terminal_n.data_ptr<float>(),
      steps.data_ptr<int64_t>(), B, P, T, H * W, (int)k, (int)n,
      (float)gamma, channels_last, current_stream());
  return {state, next, reward_n, terminal_n, steps};
}

std::vector<Tensor> framestack_gather_nstep(Tensor planes, Tensor base,
                                            Tensor left, Tensor reward,
                                            Tensor terminal, Tensor pos,
                                            int64_t k, int64_t n,
                                            double gamma,
                                            bool channels_last) {
  return framestack_gather_nstep_impl(planes, base, left, reward, terminal,
                                      pos, k, n, gamma, channels_last,
                                      nullptr);
}

std::vector<Tensor> framestack_gather_nstep_shift(
    Tensor planes, Tensor base, Tensor left, Tensor reward, Tensor terminal,
    Tensor pos, int64_t k, int64_t n, double gamma, bool channels_last,
    Tensor shift) {
  return framestack_gather_nstep_impl(planes, base, left, reward, terminal,
                                      pos, k, n, gamma, channels_last,
                                      &shift);
}

// per-step store of a vector env into the lane rings of
// DeviceVecFrameStackBuffer (framestack_vec.hip). The ring tensors,
// head and run are written in place; returns (pos [E], leaf_idx
// [E, k+1+n], leaf_w [E, k+1+n]). The kernel reduces every slot into
// its lane's row itself, so values are never inspected on the host.
std::vector<Tensor> framestack_vec_append(
    Tensor planes, Tensor reward_col, Tensor terminal_col, Tensor left,
    Tensor head, Tensor run, Tensor frame, Tensor first, Tensor reward,
    Tensor terminal, Tensor done, Tensor fill, int64_t k, int64_t n) {
  TORCH_CHECK(planes.is_cuda() && planes.scalar_type() == at::kByte &&
                  planes.is_contiguous() && planes.dim() == 3,
              "planes must be contiguous uint8 [E*R, H, W] CUDA");
  TORCH_CHECK(k >= 1 && k <= 8, "k must be in [1, 8]");
  TORCH_CHECK(n >= 1 && n <= 16, "n must be in [1, 16]");
  TORCH_CHECK(head.dim() == 1 && head.numel() >= 1,
              "head must be [E] with E >= 1");
  const int64_t E = head.numel(), G = k + n;
  const int64_t H = planes.size(1), W = planes.size(2), HW = H * W;
  TORCH_CHECK(HW > 0, "planes must not be empty");
  TORCH_CHECK(planes.size(0) % E == 0, "planes must hold E rows");
  const int64_t R = planes.size(0) / E, S = R - G;
  TORCH_CHECK(S >= 2 * G, "lane_slots must be at least 2 * (k + n)");
  check_arg(reward_col, planes, at::kFloat, E * R, "reward column");
  check_arg(terminal_col, planes, at::kFloat, E * R, "terminal column");
  check_arg(left, planes, at::kLong, E * R, "left");
  check_arg(head, planes, at::kLong, E, "head");
  check_arg(run, planes, at::kLong, E, "run");
  check_arg(frame, planes, at::kByte, E * HW, "frame");
  check_arg(reward, planes, at::kFloat, E, "reward");
  check_arg(terminal, planes, at::kFloat, E, "terminal");
  check_arg(done, planes, at::kFloat, E, "done");
  check_arg(fill, planes, at::kFloat, 1, "fill");
  TORCH_CHECK(frame.dim() == 3 && frame.size(0) == E && frame.size(1) == H &&
                  frame.size(2) == W,
              "frame must be [E, H, W]");
  TORCH_CHECK(first.is_cuda() && first.device() == planes.device() &&
                  first.scalar_type() == at::kByte && first.dim() == 4 &&
                  first.size(0) == E && first.size(1) == k &&
                  first.size(2) == H && first.size(3) == W,
              "first must be uint8 [E, k, H, W] on the ring's device");
  bool first_nhwc = false;
  if (!first.is_contiguous()) {
    TORCH_CHECK(first.is_contiguous(at::MemoryFormat::ChannelsLast),
                "first must be contiguous or in channels_last strides");
    first_nhwc = true;
  }
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(planes.device());
  const int64_t L = k + 1 + n;
  Tensor pos = at::empty({E}, head.options());
  Tensor leaf_idx = at::empty({E, L}, head.options());
  Tensor leaf_w = at::empty({E, L}, reward.options());
  framestack_vec_append_launch(
      planes.data_ptr<unsigned char>(), reward_col.data_ptr<float>(),
      terminal_col.data_ptr<float>(), left.data_ptr<int64_t>(),
      head.data_ptr<int64_t>(), run.data_ptr<int64_t>(),
      frame.data_ptr<unsigned char>(), first.data_ptr<unsigned char>(),
      reward.data_ptr<float>(), terminal.data_ptr<float>(),
      done.data_ptr<float>(), fill.data_ptr<float>(),
      pos.data_ptr<int64_t>(), leaf_idx.data_ptr<int64_t>(),
      leaf_w.data_ptr<float>(), E, S, HW, (int)k, (int)n, first_nhwc,
      current_stream());
  return {pos, leaf_idx, leaf_w};
}

// batched device PixelCatch (pixelcatch.hip). Everything is written in
// place; obs is [E, 4, 84, 84] u8, contiguous or in channels_last
// strides. Returns whether obs was taken as NHWC.
bool pixelcatch_check_env(const Tensor& state, const Tensor& ball_no,
                          const Tensor& obs) {
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kInt &&
                  state.is_contiguous() && state.dim() == 2 &&
                  state.size(1) == 10,
              "state must be contiguous int32 [E, 10] CUDA");
  const int64_t E = state.size(0);
  check_arg(ball_no, state, at::kLong, E, "ball_no");
  TORCH_CHECK(obs.is_cuda() && obs.device() == state.device() &&
                  obs.scalar_type() == at::kByte && obs.dim() == 4 &&
                  obs.size(0) == E && obs.size(1) == 4 &&
                  obs.size(2) == 84 && obs.size(3) == 84,
              "obs must be uint8 [E, 4, 84, 84] on state's device");
  const bool nhwc = obs.stride(1) == 1;
  if (nhwc) {
    TORCH_CHECK(obs.stride(0) == 28224 && obs.stride(2) == 336 &&
                    obs.stride(3) == 4,
                "obs must be contiguous or in channels_last strides");
  } else {
    TORCH_CHECK(obs.stride(0) == 28224 && obs.stride(1) == 7056 &&
                    obs.stride(2) == 84 && obs.stride(3) == 1,
                "obs must be contiguous or in channels_last strides");
  }
  TORCH_CHECK((uintptr_t)obs.data_ptr() % 16 == 0,
              "obs must be 16-byte aligned");
  return nhwc;
}

void pixelcatch_step(Tensor state, Tensor ball_no, Tensor action, Tensor obs,
                     Tensor frame, Tensor reward, Tensor done, Tensor ep_len,
                     uint64_t seed, int64_t balls, int64_t max_episode_steps,
                     bool auto_reset, c10::optional<Tensor> log_frames,
                     c10::optional<Tensor> log_action,
                     c10::optional<Tensor> log_reward,
                     c10::optional<Tensor> log_terminal) {
  const bool nhwc = pixelcatch_check_env(state, ball_no, obs);
  const int64_t E = state.size(0);
  check_arg(action, state, at::kLong, E, "action");
  check_arg(frame, state, at::kByte, E * 7056, "frame");
  check_arg(reward, state, at::kFloat, E, "reward");
  check_arg(done, state, at::kFloat, E, "done");
  check_arg(ep_len, state, at::kInt, E, "ep_len");
  TORCH_CHECK((uintptr_t)frame.data_ptr() % 16 == 0,
              "frame must be 16-byte aligned");
  TORCH_CHECK(balls >= 1 && balls <= (1 << 20), "balls must be in [1, 2^20]");
  TORCH_CHECK(max_episode_steps >= 1 && max_episode_steps <= (1 << 30),
              "max_episode_steps must be in [1, 2^30]");
  unsigned char* lf = nullptr;
  int64_t* la = nullptr;
  float* lr = nullptr;
  float* lt = nullptr;
  int64_t max_len = 0;
  if (log_frames.has_value()) {
    TORCH_CHECK(log_action.has_value() && log_reward.has_value() &&
                    log_terminal.has_value(),
                "the four log tensors come together");
    const Tensor& f = *log_frames;
    TORCH_CHECK(f.dim() == 4 && f.size(0) == E && f.size(1) > 4 &&
                    f.size(2) == 84 && f.size(3) == 84,
                "log_frames must be [E, max_len + 4, 84, 84]");
    max_len = f.size(1) - 4;
    TORCH_CHECK(max_len <= (1 << 30), "log too long");
    check_arg(f, state, at::kByte, E * (max_len + 4) * 7056, "log_frames");
    check_arg(*log_action, state, at::kLong, E * max_len, "log_action");
    check_arg(*log_reward, state, at::kFloat, E * max_len, "log_reward");
    check_arg(*log_terminal, state, at::kFloat, E * max_len,
              "log_terminal");
    TORCH_CHECK((uintptr_t)f.data_ptr() % 16 == 0,
                "log_frames must be 16-byte aligned");
    lf = f.data_ptr<unsigned char>();
    la = log_action->data_ptr<int64_t>();
    lr = log_reward->data_ptr<float>();
    lt = log_terminal->data_ptr<float>();
  }
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(state.device());
  pixelcatch_step_launch(
      state.data_ptr<int32_t>(), ball_no.data_ptr<int64_t>(),
      action.data_ptr<int64_t>(), obs.data_ptr<unsigned char>(),
      frame.data_ptr<unsigned char>(), reward.data_ptr<float>(),
      done.data_ptr<float>(), ep_len.data_ptr<int32_t>(), lf, la, lr, lt, E,
      seed, (int)balls, (int)max_episode_steps, (int)max_len, auto_reset,
      nhwc, current_stream());
}

void pixelcatch_reset(Tensor state, Tensor ball_no, Tensor mask, Tensor obs,
                      uint64_t seed, int64_t balls) {
  const bool nhwc = pixelcatch_check_env(state, ball_no, obs);
  const int64_t E = state.size(0);
  check_arg(mask, state, at::kByte, E, "mask");
  TORCH_CHECK(balls >= 1 && balls <= (1 << 20), "balls must be in [1, 2^20]");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(state.device());
  pixelcatch_reset_launch(state.data_ptr<int32_t>(),
                          ball_no.data_ptr<int64_t>(),
                          mask.data_ptr<unsigned char>(),
                          obs.data_ptr<unsigned char>(), E, seed, (int)balls,
                          nhwc, current_stream());
}

// Argument checks shared by the four stem conv entry points. The
// kernels index a frame as 84 x 84 pixels of 4 bytes without looking at
// the tensor's sizes, so anything else must stop here.
void check_stem_frames(const Tensor& frames) {
  TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kByte &&
                  frames.is_contiguous(),
              "frames must be contiguous u8 CUDA");
  TORCH_CHECK(frames.dim() == 4 && frames.size(1) == 84 &&
                  frames.size(2) == 84 && frames.size(3) == 4,
              "frames must be [B, 84, 84, 4] (NHWC)");
}

// weight: [256, 32] bf16 patch-major repack; bias: [32] fp32 or empty.
// Both on the frames' device. Returns the bias pointer or nullptr.
const float* check_stem_weight_bias(const Tensor& frames,
                                    const Tensor& weight,
                                    const Tensor& bias) {
  TORCH_CHECK(weight.is_cuda() && weight.scalar_type() == at::kBFloat16 &&
                  weight.is_contiguous() && weight.dim() == 2 &&
                  weight.size(0) == 256 && weight.size(1) == 32,
              "weight must be contiguous [256,32] bf16 CUDA");
  TORCH_CHECK(weight.device() == frames.device(),
              "weight must be on the frames' device");
  if (!bias.defined() || bias.numel() == 0) return nullptr;
  TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == at::kFloat &&
                  bias.is_contiguous() && bias.dim() == 1 &&
                  bias.size(0) == 32,
              "bias must be contiguous [32] fp32 CUDA, or empty");
  TORCH_CHECK(bias.device() == frames.device(),
              "bias must be on the frames' device");
  return bias.data_ptr<float>();
}

void check_stem_dy(const Tensor& dy, const Tensor& frames) {
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
                  dy.is_contiguous() && dy.dim() == 2 && dy.size(1) == 32,
              "dy must be contiguous [K,32] bf16 CUDA");
  check_stem_frames(frames);
  TORCH_CHECK(frames.device() == dy.device(),
              "frames must be on dy's device");
  TORCH_CHECK(dy.size(0) == frames.size(0) * 400,
              "K must equal batch*400");
}

std::vector<Tensor> conv1_wrw(Tensor dy, Tensor frames, double scale) {
  // dy: [K, 32] bf16 (NHWC-flattened conv output grad);
  // frames: [B, 84, 84, 4] u8. Returns [32, 4, 8, 8] fp32 grad.
  check_stem_dy(dy, frames);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dy.device());
  if (dy.size(0) == 0) {  // no frames: zero gradients, nothing to launch
    return {at::zeros({32, 4, 8, 8}, dy.options().dtype(at::kFloat)),
            at::zeros({32}, dy.options().dtype(at::kFloat))};
  }
  Tensor scratch = at::empty({32 * 256},
                             dy.options().dtype(at::kFloat));
  Tensor grad_w = at::empty({32, 4, 8, 8},
                            dy.options().dtype(at::kFloat));
  Tensor grad_b = at::empty({32}, dy.options().dtype(at::kFloat));
  conv1_wrw_launch(dy.data_ptr(), frames.data_ptr<unsigned char>(),
                   scratch.data_ptr<float>(), grad_w.data_ptr<float>(),
                   grad_b.data_ptr<float>(), dy.size(0), (float)scale,
                   current_stream());
  return {grad_w, grad_b};
}

Tensor conv1_fwd(Tensor frames, Tensor weight, Tensor bias,
                 double scale) {
  // frames: [B, 84, 84, 4] u8 NHWC; weight: [256, 32] bf16 (patch-major
  // repack of the conv weight); bias: [32] fp32 or empty.
  check_stem_frames(frames);
  const float* bias_ptr = check_stem_weight_bias(frames, weight, bias);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(frames.device());
  int64_t K = frames.size(0) * 400;
  Tensor out = at::empty({K, 32},
                         weight.options().dtype(at::kBFloat16));
  if (K == 0) return out;  // no frames: nothing to launch
  conv1_fwd_launch(frames.data_ptr<unsigned char>(), weight.data_ptr(),
                   bias_ptr, out.data_ptr(), K, (float)scale,
                   current_stream());
  return out;
}

// Fused-activation stem forward: returns {relu(conv + bias) as [K, 32]
// bf16, sign mask [K] int32 (bit c of word k set <=> y[k][c] > 0)}.
std::vector<Tensor> conv1_fwd_relu(Tensor frames, Tensor weight,
                                   Tensor bias, double scale) {
  check_stem_frames(frames);
  const float* bias_ptr = check_stem_weight_bias(frames, weight, bias);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(frames.device());
  int64_t K = frames.size(0) * 400;
  Tensor out = at::empty({K, 32},
                         weight.options().dtype(at::kBFloat16));
  Tensor mask = at::empty({K}, weight.options().dtype(at::kInt));
  if (K == 0) return {out, mask};  // no frames: nothing to launch
  conv1_fwd_relu_launch(frames.data_ptr<unsigned char>(),
                        weight.data_ptr(), bias_ptr, out.data_ptr(),
                        (unsigned int*)mask.data_ptr<int>(), K,
                        (float)scale, current_stream());
  return {out, mask};
}

// Weight/bias gradient of the fused-activation stem: dy is the
// gradient w.r.t. the ACTIVATED output; elements whose mask bit is
// clear are zeroed as they are loaded.
std::vector<Tensor> conv1_wrw_masked(Tensor dy, Tensor mask, Tensor frames,
                                     double scale) {
  check_stem_dy(dy, frames);
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == at::kInt &&
                  mask.is_contiguous() && mask.dim() == 1 &&
                  mask.size(0) == dy.size(0),
              "mask must be contiguous [K] int32 CUDA");
  TORCH_CHECK(mask.device() == dy.device(),
              "mask must be on dy's device");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dy.device());
  if (dy.size(0) == 0) {  // no frames: zero gradients, nothing to launch
    return {at::zeros({32, 4, 8, 8}, dy.options().dtype(at::kFloat)),
            at::zeros({32}, dy.options().dtype(at::kFloat))};
  }
  TORCH_CHECK((uintptr_t)mask.data_ptr() % 16 == 0,
              "mask must be 16-byte aligned");
  Tensor scratch = at::empty({32 * 256},
                             dy.options().dtype(at::kFloat));
  Tensor grad_w = at::empty({32, 4, 8, 8},
                            dy.options().dtype(at::kFloat));
  Tensor grad_b = at::empty({32}, dy.options().dtype(at::kFloat));
  conv1_wrw_masked_launch(dy.data_ptr(),
                          (const unsigned int*)mask.data_ptr<int>(),
                          frames.data_ptr<unsigned char>(),
                          scratch.data_ptr<float>(),
                          grad_w.data_ptr<float>(),
                          grad_b.data_ptr<float>(), dy.size(0),
                          (float)scale, current_stream());
  return {grad_w, grad_b};
}

void check_rows_bf16(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                  t.dim() == 2 && t.is_contiguous(),
              name, " must be a contiguous [R, C] bf16 CUDA tensor");
  TORCH_CHECK(t.size(1) % 8 == 0 && t.size(1) >= 8 && t.size(1) <= 2048,
              name, ": C must be a multiple of 8 in [8, 2048]");
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, name,
              " must be 16-byte aligned");
}

// In place on the NHWC [R, C] view of a channels-last activation:
// y = relu(bf16(y + bf16(bias[c]))).
void bias_relu_(Tensor y, Tensor bias) {
  check_rows_bf16(y, "y");
  check_f32_cuda(bias, "bias");
  TORCH_CHECK(bias.numel() == y.size(1), "bias must have C elements");
  TORCH_CHECK((uintptr_t)bias.data_ptr() % 16 == 0,
              "bias must be 16-byte aligned");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y.device());
  bias_relu_launch(y.data_ptr(), bias.data_ptr<float>(), y.size(0),
                   (int)y.size(1), current_stream());
}

// {gx = y > 0 ? gy : 0 as [R, C] bf16, per-channel sum of gx rounded to
// bf16 and returned as fp32 [C]}; the sum is deterministic.
std::vector<Tensor> bias_relu_bwd(Tensor gy, Tensor y) {
  check_rows_bf16(gy, "gy");
  check_rows_bf16(y, "y");
  TORCH_CHECK(gy.sizes() == y.sizes(), "gy and y must have equal shapes");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(gy.device());
  const int64_t R = gy.size(0);
  const int C = (int)gy.size(1);
  Tensor gx = at::empty_like(gy);
  Tensor partial = at::empty({bias_relu_bwd_blocks(R, C), C},
                             gy.options().dtype(at::kFloat));
  Tensor grad_bias = at::empty({C}, gy.options().dtype(at::kFloat));
  bias_relu_bwd_launch(gy.data_ptr(), y.data_ptr(), gx.data_ptr(),
                       partial.data_ptr<float>(),
                       grad_bias.data_ptr<float>(), R, C,
                       current_stream());
  return {gx, grad_bias};
}

void check_flat_bf16(const Tensor& t, int64_t N, int64_t C, int64_t HW,
                     const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                  t.is_contiguous() && t.numel() == N * C * HW,
              name, " must be a contiguous bf16 CUDA tensor of N*C*HW");
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= 2048 && HW >= 1 &&
                  C * HW <= 32768,
              name, ": C must be a multiple of 8 in [8, 2048] and one "
              "sample (C*HW bf16) must fit 64 KB of LDS");
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, name,
              " must be 16-byte aligned");
}

// relu(bf16(y + bf16(bias[c]))) of the NHWC rows y [N*HW, C], written
// as the NCHW-flat matrix [N, C*HW] (what nn.Flatten makes of the
// channels-last activation).
Tensor bias_relu_flat(Tensor y, Tensor bias, int64_t N) {
  check_rows_bf16(y, "y");
  TORCH_CHECK(N > 0 && y.size(0) % N == 0, "rows must be N*HW");
  const int64_t C = y.size(1), HW = y.size(0) / N;
  check_flat_bf16(y, N, C, HW, "y");
  check_f32_cuda(bias, "bias");
  TORCH_CHECK(bias.numel() == C, "bias must have C elements");
  TORCH_CHECK((uintptr_t)bias.data_ptr() % 16 == 0,
              "bias must be 16-byte aligned");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y.device());
  Tensor out = at::empty({N, C * HW}, y.options());
  bias_relu_flat_launch(y.data_ptr(), bias.data_ptr<float>(),
                        out.data_ptr(), N, (int)C, (int)HW,
                        current_stream());
  return out;
}

// Backward of bias_relu_flat: gy and the saved activation y are both
// NCHW-flat [N, C*HW]; returns {gx as NHWC rows [N*HW, C], bias
// gradient (deterministic, bf16-rounded) as fp32 [C]}.
std::vector<Tensor> bias_relu_flat_bwd(Tensor gy, Tensor y, int64_t C) {
  TORCH_CHECK(gy.dim() == 2 && y.dim() == 2 && gy.sizes() == y.sizes(),
              "gy and y must be [N, C*HW] of equal shape");
  const int64_t N = gy.size(0);
  TORCH_CHECK(N > 0 && C > 0 && gy.size(1) % C == 0,
              "row length must be C*HW");
  const int64_t HW = gy.size(1) / C;
  check_flat_bf16(gy, N, C, HW, "gy");
  check_flat_bf16(y, N, C, HW, "y");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(gy.device());
  Tensor gx = at::empty({N * HW, C}, gy.options());
  Tensor partial = at::empty({bias_relu_flat_blocks(N), C},
                             gy.options().dtype(at::kFloat));
  Tensor grad_bias = at::empty({C}, gy.options().dtype(at::kFloat));
  bias_relu_flat_bwd_launch(gy.data_ptr(), y.data_ptr(), gx.data_ptr(),
                            partial.data_ptr<float>(),
                            grad_bias.data_ptr<float>(), N, (int)C,
                            (int)HW, current_stream());
  return {gx, grad_bias};
}

Tensor tr16_probe(int64_t mode) {
  Tensor out = at::empty({64, 4}, at::TensorOptions()
                                      .dtype(at::kFloat)
                                      .device(at::kCUDA));
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(out.device());
  tr16_probe_launch(out.data_ptr<float>(), (int)mode, current_stream());
  return out;
}

Tensor fwd_bfrag_probe(int64_t which) {
  Tensor out = at::empty({2, 256, 8}, at::TensorOptions()
                                          .dtype(at::kFloat)
                                          .device(at::kCUDA));
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(out.device());
  fwd_bfrag_probe_launch(out.data_ptr<float>(), (int)which,
                         current_stream());
  return out;
}

Tensor tr16_diag(int64_t mode) {
  int64_t n = mode <= 1 ? 8192 : 4096;
  Tensor out = at::empty({n}, at::TensorOptions()
                                  .dtype(at::kFloat)
                                  .device(at::kCUDA));
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(out.device());
  tr16_diag_launch(out.data_ptr<float>(), (int)mode, current_stream());
  return out;
}

Tensor mfma_probe(Tensor A, Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16 &&
              A.is_contiguous() && A.size(0) == 16 && A.size(1) == 32,
              "A must be [16,32] bf16");
  TORCH_CHECK(B.is_contiguous() && B.size(0) == 32 && B.size(1) == 16,
              "B must be [32,16] bf16");
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(A.device());
  Tensor D = at::empty({16, 16}, A.options().dtype(at::kFloat));
  mfma_probe_launch(A.data_ptr(), B.data_ptr(), D.data_ptr<float>(),
                    current_stream());
  return D;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "machin_amd gfx950 HIP kernels";
  m.def("sumtree_update", &sumtree_update);
  m.def("sumtree_build", &sumtree_build);
  m.def("sumtree_sample", &sumtree_sample);
  m.def("discounted_returns", &discounted_returns);
  m.def("gae", &gae);
  m.def("vtrace", &vtrace);
  m.def("vtrace_bt", &vtrace_bt);
  m.def("categorical_projection", &categorical_projection);
  m.def("c51_loss_fwd", &c51_loss_fwd);
  m.def("c51_loss_bwd", &c51_loss_bwd);
  m.def("noisy_linear_fwd", &noisy_linear_fwd);
  m.def("noisy_linear_bwd_input", &noisy_linear_bwd_input);
  m.def("noisy_linear_bwd_weight", &noisy_linear_bwd_weight);
  m.def("factorised_noise_", &factorised_noise_);
  m.def("noisy_linear_slices", &noisy_linear_slices_py);
  m.def("multi_tensor_polyak", &multi_tensor_polyak);
  m.def("multi_tensor_polyak_cached", &multi_tensor_polyak_cached);
  m.def("fused_rmsprop_cached", &fused_rmsprop_cached);
  m.def("nstep_returns", &nstep_returns);
  m.def("gaussian_sample_logprob", &gaussian_sample_logprob);
  m.def("gaussian_logprob", &gaussian_logprob);
  m.def("normal_noise_", &normal_noise_);
  m.def("ou_update_", &ou_update_);
  m.def("u8_to_bf16_scale", &u8_to_bf16_scale);
  m.def("framestack_gather", &framestack_gather);
  m.def("framestack_gather_nstep", &framestack_gather_nstep);
  m.def("framestack_gather_shift", &framestack_gather_shift);
  m.def("framestack_gather_nstep_shift", &framestack_gather_nstep_shift);
  m.def("framestack_vec_append", &framestack_vec_append);
  m.def("pixelcatch_step", &pixelcatch_step);
  m.def("pixelcatch_reset", &pixelcatch_reset);
  m.def("pg_head_fwd", &pg_head_fwd);
  m.def("pg_head_bwd", &pg_head_bwd);
  m.def("conv1_wrw", &conv1_wrw);
  m.def("mfma_probe", &mfma_probe);
  m.def("tr16_probe", &tr16_probe);
  m.def("fwd_bfrag_probe", &fwd_bfrag_probe);
  m.def("tr16_diag", &tr16_diag);
  m.def("conv1_fwd", &conv1_fwd);
  m.def("conv1_fwd_relu", &conv1_fwd_relu);
  m.def("conv1_wrw_masked", &conv1_wrw_masked);
  m.def("bias_relu_", &bias_relu_);
  m.def("bias_relu_bwd", &bias_relu_bwd);
  m.def("bias_relu_flat", &bias_relu_flat);
  m.def("bias_relu_flat_bwd", &bias_relu_flat_bwd);
}
