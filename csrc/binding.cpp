// torch.ops.bllm.* registration for the gfx950 kernel library.
//
// Every op validates shapes/dtypes on the host before launching (a bad launch on the shared
// GPU pool can reset the node), allocates outputs through the PyTorch HIP caching allocator
// and launches on the current HIP stream, so ops compose with torch streams, events and
// hipGraph capture.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>
#include <hipblaslt/hipblaslt.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

#include "common.h"
#include "api.h"

using at::Tensor;
using c10::optional;
using bllm::DType;

namespace {

DType dt_of(const Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return DType::F32;
    case at::kBFloat16: return DType::BF16;
    case at::kHalf: return DType::F16;
    default: TORCH_CHECK(false, "bllm: unsupported dtype ", t.scalar_type());
  }
  return DType::F32;
}

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_gpu(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "bllm: ", name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), "bllm: ", name, " must be contiguous");
}

void check_rows(const Tensor& x, int64_t vec_elems) {
  TORCH_CHECK(x.dim() == 2, "bllm: expected a 2-D [rows, dim] tensor");
  TORCH_CHECK(x.size(1) % vec_elems == 0, "bllm: row length ", x.size(1), " must be a multiple of ", vec_elems);
}

// ------------------------------------------------------------------ norms
std::tuple<Tensor, Tensor> rmsnorm_fwd(const Tensor& x, const Tensor& w, double eps) {
  check_gpu(x, "x"); check_gpu(w, "w");
  c10::DeviceGuard g(x.device());
  check_rows(x, 16 / x.element_size());
  const int64_t N = x.size(0), d = x.size(1);
  TORCH_CHECK(d <= bllm::norm_max_dim(dt_of(x)) && w.numel() == d && w.scalar_type() == x.scalar_type());
  auto y = at::empty_like(x);
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  bllm::rmsnorm_fwd(dt_of(x), x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr<float>(), N, d, (float)eps,
                    (long)d, stream());
  return {y, rstd};
}

// y: a [N, d] row-strided view (stride(0) >= d, 16-B aligned rows), e.g. the x part of a
// K-augmented LoRA operand [x | s t]; returns rstd
Tensor rmsnorm_fwd_into_(const Tensor& x, const Tensor& w, double eps, Tensor& y) {
  check_gpu(x, "x"); check_gpu(w, "w");
  TORCH_CHECK(y.is_cuda() && y.device() == x.device(), "rmsnorm_fwd_into_: y must be on x's GPU");
  c10::DeviceGuard g(x.device());
  check_rows(x, 16 / x.element_size());
  const int64_t N = x.size(0), d = x.size(1);
  TORCH_CHECK(d <= bllm::norm_max_dim(dt_of(x)) && w.numel() == d && w.scalar_type() == x.scalar_type());
  TORCH_CHECK(y.dim() == 2 && y.size(0) == N && y.size(1) == d && y.stride(1) == 1 && y.stride(0) >= d &&
                  y.scalar_type() == x.scalar_type() && (y.stride(0) * y.element_size()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(y.data_ptr()) % 16 == 0,
              "rmsnorm_fwd_into_: y must be a 16-B aligned [N, d] row-strided view");
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  bllm::rmsnorm_fwd(dt_of(x), x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr<float>(), N, d, (float)eps,
                    (long)y.stride(0), stream());
  return rstd;
}

// dW goes to `dw_out` (any float dtype, written or accumulated) when given, else a new fp32 [d]
static Tensor vec_out(const optional<Tensor>& o, const Tensor& x, int64_t d, const char* name) {
  if (o.has_value()) {
    check_gpu(*o, name);
    TORCH_CHECK(o->numel() == d, "bllm: ", name, " must have ", d, " elements");
    return *o;
  }
  return at::empty({d}, x.options().dtype(at::kFloat));
}

std::tuple<Tensor, Tensor> rmsnorm_bwd(const Tensor& dy, const Tensor& x, const Tensor& w, const Tensor& rstd,
                                       const optional<Tensor>& dx_acc, const optional<Tensor>& dw_out,
                                       bool accumulate) {
  check_gpu(dy, "dy"); check_gpu(x, "x"); check_gpu(w, "w"); check_gpu(rstd, "rstd");
  c10::DeviceGuard g(x.device());
  check_rows(x, 16 / x.element_size());
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.scalar_type() == x.scalar_type());
  const int64_t N = x.size(0), d = x.size(1);
  TORCH_CHECK(d <= bllm::norm_max_dim(dt_of(x)) && w.numel() == d);
  const void* acc = nullptr;
  if (dx_acc.has_value()) {
    check_gpu(*dx_acc, "dx_acc");
    TORCH_CHECK(dx_acc->sizes() == x.sizes() && dx_acc->scalar_type() == x.scalar_type());
    acc = dx_acc->data_ptr();
  }
  auto dx = at::empty_like(x);
  const int nwg = bllm::norm_bwd_num_wg(N, d);
  auto part = at::empty({nwg, d}, x.options().dtype(at::kFloat));
  Tensor dw = vec_out(dw_out, x, d, "dw_out");
  bllm::rmsnorm_bwd(dt_of(x), dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr<float>(), acc, dx.data_ptr(),
                    part.data_ptr<float>(), dt_of(dw), dw.data_ptr(), accumulate && dw_out.has_value(), N, d, nwg,
                    stream());
  return {dx, dw};
}

std::tuple<Tensor, Tensor, Tensor> layernorm_fwd(const Tensor& x, const Tensor& w, const Tensor& b, double eps) {
  check_gpu(x, "x"); check_gpu(w, "w"); check_gpu(b, "b");
  c10::DeviceGuard g(x.device());
  check_rows(x, 16 / x.element_size());
  const int64_t N = x.size(0), d = x.size(1);
  TORCH_CHECK(d <= bllm::norm_max_dim(dt_of(x)) && w.numel() == d && b.numel() == d);
  auto y = at::empty_like(x);
  auto mean = at::empty({N}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  bllm::layernorm_fwd(dt_of(x), x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr<float>(),
                      rstd.data_ptr<float>(), N, d, (float)eps, stream());
  return {y, mean, rstd};
}

std::tuple<Tensor, Tensor, Tensor> layernorm_bwd(const Tensor& dy, const Tensor& x, const Tensor& w,
                                                 const Tensor& mean, const Tensor& rstd,
                                                 const optional<Tensor>& dx_acc, const optional<Tensor>& dw_out,
                                                 const optional<Tensor>& db_out, bool accumulate) {
  check_gpu(dy, "dy"); check_gpu(x, "x"); check_gpu(w, "w");
  c10::DeviceGuard g(x.device());
  check_rows(x, 16 / x.element_size());
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.scalar_type() == x.scalar_type());
  const int64_t N = x.size(0), d = x.size(1);
  TORCH_CHECK(d <= bllm::norm_max_dim(dt_of(x)) && w.numel() == d);
  const void* acc = nullptr;
  if (dx_acc.has_value()) {
    check_gpu(*dx_acc, "dx_acc");
    TORCH_CHECK(dx_acc->sizes() == x.sizes() && dx_acc->scalar_type() == x.scalar_type());
    acc = dx_acc->data_ptr();
  }
  auto dx = at::empty_like(x);
  const int nwg = bllm::norm_bwd_num_wg(N, d);
  auto pw = at::empty({nwg, d}, x.options().dtype(at::kFloat));
  auto pb = at::empty({nwg, d}, x.options().dtype(at::kFloat));
  TORCH_CHECK(dw_out.has_value() == db_out.has_value(), "layernorm_bwd: give both dw_out and db_out or neither");
  Tensor dw = vec_out(dw_out, x, d, "dw_out");
  Tensor db = vec_out(db_out, x, d, "db_out");
  TORCH_CHECK(dw.scalar_type() == db.scalar_type(), "layernorm_bwd: dw_out / db_out dtypes differ");
  bllm::layernorm_bwd(dt_of(x), dy.data_ptr(), x.data_ptr(), w.data_ptr(), mean.data_ptr<float>(),
                      rstd.data_ptr<float>(), acc, dx.data_ptr(), pw.data_ptr<float>(), pb.data_ptr<float>(),
                      dt_of(dw), dw.data_ptr(), db.data_ptr(), accumulate && dw_out.has_value(), N, d, nwg,
                      stream());
  return {dx, dw, db};
}

// x2 = x + dropout(a), (y, mean, rstd) = LayerNorm(x2): one pass (GPT-2's attention residual + norm2)
std::tuple<Tensor, Tensor, Tensor, Tensor> dropout_add_layernorm(const Tensor& x, const Tensor& a, const Tensor& w,
                                                                 const Tensor& b, double eps, double p, int64_t seed,
                                                                 int64_t offset) {
  check_gpu(x, "x"); check_gpu(a, "a"); check_gpu(w, "w"); check_gpu(b, "b");
  c10::DeviceGuard g(x.device());
  check_rows(x, 16 / x.element_size());
  TORCH_CHECK(a.sizes() == x.sizes() && a.scalar_type() == x.scalar_type() && a.is_contiguous(),
              "dropout_add_layernorm: a must be a contiguous tensor of x's shape and dtype");
  const int64_t N = x.size(0), d = x.size(1);
  TORCH_CHECK(d <= bllm::norm_max_dim(dt_of(x)) && w.numel() == d && b.numel() == d &&
              w.scalar_type() == x.scalar_type() && b.scalar_type() == x.scalar_type());
  auto x2 = at::empty_like(x);
  auto y = at::empty_like(x);
  auto mean = at::empty({N}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  bllm::dropout_add_layernorm_fwd(dt_of(x), x.data_ptr(), a.data_ptr(), x2.data_ptr(), w.data_ptr(), b.data_ptr(),
                                  y.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(), N, d, (float)eps,
                                  (float)p, (uint64_t)seed, (uint64_t)offset, stream());
  return {x2, y, mean, rstd};
}

// ------------------------------------------------------------------ elementwise
Tensor dropout_add(const Tensor& x, const Tensor& a, double p, int64_t seed, int64_t offset) {
  check_gpu(x, "x"); check_gpu(a, "a");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.sizes() == a.sizes() && x.scalar_type() == a.scalar_type());
  auto out = at::empty_like(x);
  bllm::dropout_add(dt_of(x), x.data_ptr(), a.data_ptr(), out.data_ptr(), x.numel(), (float)p, (uint64_t)seed,
                    (uint64_t)offset, stream());
  return out;
}

Tensor dropout_bwd(const Tensor& dy, double p, int64_t seed, int64_t offset) {
  check_gpu(dy, "dy");
  c10::DeviceGuard g(dy.device());
  auto out = at::empty_like(dy);
  bllm::dropout_add(dt_of(dy), nullptr, dy.data_ptr(), out.data_ptr(), dy.numel(), (float)p, (uint64_t)seed,
                    (uint64_t)offset, stream());
  return out;
}

Tensor transpose2d(const Tensor& a) {
  check_gpu(a, "a");
  c10::DeviceGuard g(a.device());
  TORCH_CHECK(a.dim() == 2 && a.is_contiguous() && a.element_size() == 2, "transpose2d: contiguous 2-D 16-bit tensor");
  const int64_t R = a.size(0), C = a.size(1);
  TORCH_CHECK(R % 8 == 0 && C % 8 == 0, "transpose2d: both dims must be multiples of 8");
  auto out = at::empty({C, R}, a.options());
  bllm::transpose16(a.data_ptr(), out.data_ptr(), R, C, stream());
  return out;
}

Tensor swiglu_fwd(const Tensor& gu) {
  check_gpu(gu, "gu");
  c10::DeviceGuard g(gu.device());
  TORCH_CHECK(gu.dim() == 2 && gu.size(1) % 2 == 0);
  const int64_t N = gu.size(0), F = gu.size(1) / 2;
  auto act = at::empty({N, F}, gu.options());
  bllm::swiglu_fwd(dt_of(gu), gu.data_ptr(), act.data_ptr(), N, F, (long)F, stream());
  return act;
}

// act: a [N, F] row-strided view (the act part of a K-augmented [act | s t] operand)
void swiglu_fwd_into_(const Tensor& gu, Tensor& act) {
  check_gpu(gu, "gu");
  TORCH_CHECK(act.is_cuda() && act.device() == gu.device(), "swiglu_fwd_into_: act must be on gu's GPU");
  c10::DeviceGuard g(gu.device());
  TORCH_CHECK(gu.dim() == 2 && gu.size(1) % 2 == 0 && gu.is_contiguous());
  const int64_t N = gu.size(0), F = gu.size(1) / 2;
  TORCH_CHECK(act.dim() == 2 && act.size(0) == N && act.size(1) == F && act.stride(1) == 1 && act.stride(0) >= F &&
                  act.scalar_type() == gu.scalar_type(),
              "swiglu_fwd_into_: act must be an [N, F] row-strided view");
  bllm::swiglu_fwd(dt_of(gu), gu.data_ptr(), act.data_ptr(), N, F, (long)act.stride(0), stream());
}

Tensor swiglu_bwd(const Tensor& gu, const Tensor& dact) {
  check_gpu(gu, "gu"); check_gpu(dact, "dact");
  c10::DeviceGuard g(gu.device());
  const int64_t N = gu.size(0), F = gu.size(1) / 2;
  TORCH_CHECK(dact.size(0) == N && dact.size(1) == F && dact.scalar_type() == gu.scalar_type());
  auto dgu = at::empty_like(gu);
  bllm::swiglu_bwd(dt_of(gu), gu.data_ptr(), dact.data_ptr(), dgu.data_ptr(), nullptr, N, F, stream());
  return dgu;
}

// swiglu_bwd with dact = base + scale . u P (base [N, F] and u [N, r] row-strided views, P [r, F])
Tensor swiglu_bwd_lowrank(const Tensor& gu, const Tensor& base, const Tensor& u, const Tensor& P, double scale) {
  check_gpu(gu, "gu"); check_gpu(P, "P");
  c10::DeviceGuard g(gu.device());
  const int64_t N = gu.size(0), F = gu.size(1) / 2, r = P.size(0);
  TORCH_CHECK(bllm::swiglu_bwd_lr_ok((int)r, (int)F) && P.size(1) == F, "swiglu_bwd_lowrank: rank 16, F % 8");
  TORCH_CHECK(base.is_cuda() && base.dim() == 2 && base.size(0) == N && base.size(1) == F && base.stride(1) == 1 &&
                  base.stride(0) % 8 == 0 && (uintptr_t)base.data_ptr() % 16 == 0, "swiglu_bwd_lowrank: base");
  TORCH_CHECK(u.is_cuda() && u.dim() == 2 && u.size(0) == N && u.size(1) == r && u.stride(1) == 1, "swiglu_bwd_lowrank: u");
  TORCH_CHECK(base.scalar_type() == gu.scalar_type() && u.scalar_type() == gu.scalar_type() &&
                  P.scalar_type() == gu.scalar_type(), "swiglu_bwd_lowrank: dtypes");
  TORCH_CHECK(gu.scalar_type() == at::kBFloat16 || gu.scalar_type() == at::kHalf, "swiglu_bwd_lowrank: bf16 / fp16");
  TORCH_CHECK(gu.is_contiguous() && P.is_contiguous(), "swiglu_bwd_lowrank: contiguous gu and P");
  auto dgu = at::empty_like(gu);
  bllm::swiglu_bwd_lr(dt_of(gu), gu.data_ptr(), base.data_ptr(), base.stride(0), u.data_ptr(), u.stride(0),
                      P.data_ptr(), (int)r, (float)scale, dgu.data_ptr(), N, (int)F, stream());
  return dgu;
}

// swiglu_bwd_lowrank that also accumulates the LoRA gradients reading the same rows:
// gB_gate (+)= st[:, :16]^T dg, gB_up (+)= st[:, 16:32]^T du (the gate/up group's dB, st = s t), and
// gA_down_t (+)= scale u^T act (the down projection's dA, a [16, F] view of its [F, 16] gradient)
Tensor swiglu_bwd_lowrank_wgrad(const Tensor& gu, const Tensor& base, const Tensor& u, const Tensor& P, double scale,
                                const Tensor& st, Tensor& gB_gate, Tensor& gB_up, Tensor& gA_down_t, bool accumulate) {
  check_gpu(gu, "gu"); check_gpu(P, "P");
  c10::DeviceGuard g(gu.device());
  const int64_t N = gu.size(0), F = gu.size(1) / 2, r = P.size(0);
  TORCH_CHECK(bllm::swiglu_bwd_lr_wgrad_ok((int)r, (int)F) && P.size(1) == F, "swiglu_bwd_lowrank_wgrad: rank 16, F % 64");
  TORCH_CHECK(gu.scalar_type() == at::kBFloat16 || gu.scalar_type() == at::kHalf, "swiglu_bwd_lowrank_wgrad: bf16 / fp16");
  TORCH_CHECK(gu.is_contiguous() && P.is_contiguous(), "swiglu_bwd_lowrank_wgrad: contiguous gu and P");
  auto rows16 = [&](const Tensor& t, int64_t cols, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.size(0) == N && t.size(1) >= cols && t.stride(1) == 1 &&
                    (t.stride(0) * t.element_size()) % 16 == 0 && (uintptr_t)t.data_ptr() % 16 == 0 &&
                    t.scalar_type() == gu.scalar_type(),
                "swiglu_bwd_lowrank_wgrad: ", name, " must be a 16-B aligned row-strided [N, >=", cols, "] view");
  };
  rows16(base, F, "base");
  TORCH_CHECK(base.size(1) == F, "swiglu_bwd_lowrank_wgrad: base is [N, F]");
  rows16(u, 16, "u");
  rows16(st, 32, "st");
  const DType odt = dt_of(gB_gate);
  const Tensor* gs[3] = {&gB_gate, &gB_up, &gA_down_t};
  for (const Tensor* t : gs)
    TORCH_CHECK(t->is_cuda() && t->dim() == 2 && t->size(0) == 16 && t->size(1) == F && dt_of(*t) == odt &&
                    (t->is_contiguous() || t->t().is_contiguous()),
                "swiglu_bwd_lowrank_wgrad: gradients are [16, F] (transposed) contiguous blocks of one dtype");
  auto dgu = at::empty_like(gu);
  const int S = bllm::swiglu_bwd_lr_wgrad_splits(N, (int)F);
  auto part = at::empty({S, 3 * 16 * F}, gu.options().dtype(at::kFloat));
  bllm::swiglu_bwd_lr_wgrad(dt_of(gu), gu.data_ptr(), base.data_ptr(), base.stride(0), u.data_ptr(), u.stride(0),
                            P.data_ptr(), st.data_ptr(), st.stride(0), (float)scale, dgu.data_ptr(),
                            part.data_ptr<float>(), N, (int)F, S, stream());
  bllm::LoraWgradArgs a{};
  a.accumulate = accumulate;
  a.n = 3;
  for (int m = 0; m < 3; ++m) {
    a.r[m] = 16; a.len[m] = (int)F; a.sa[m] = gs[m]->stride(0); a.sb[m] = gs[m]->stride(1);
    a.gt[m][0] = gs[m]->data_ptr();
    a.part_off[m] = (int64_t)m * 16 * F;
  }
  a.part = part.data_ptr<float>(); a.part_ld = 3 * 16 * F;
  bllm::lora_reduce(odt, a, S, stream());
  return dgu;
}

// LoRA head backward of one logits-gradient chunk dl [R, V]: u = dl B^T (written to u [R, 16]) and
// gB (+)= st^T dl (gB [16, V], or a transposed view of a [V, 16] block) in one pass over dl
void lora_head_bwd_(const Tensor& dl, const Tensor& st, const Tensor& B, Tensor& u, Tensor& gB, bool accumulate) {
  check_gpu(dl, "dl"); check_gpu(B, "B");
  c10::DeviceGuard g(dl.device());
  const int64_t R = dl.size(0), V = dl.size(1);
  TORCH_CHECK(dl.scalar_type() == at::kBFloat16 || dl.scalar_type() == at::kHalf, "lora_head_bwd: bf16 / fp16");
  TORCH_CHECK(V % 64 == 0 && B.dim() == 2 && B.size(0) == 16 && B.size(1) == V, "lora_head_bwd: B is [16, V], V % 64");
  auto rows16 = [&](const Tensor& t, int64_t rows, int64_t cols, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.size(0) == rows && t.size(1) == cols && t.stride(1) == 1 &&
                    (t.stride(0) * t.element_size()) % 16 == 0 && (uintptr_t)t.data_ptr() % 16 == 0 &&
                    t.scalar_type() == dl.scalar_type(),
                "lora_head_bwd: ", name, " must be a 16-B aligned row-strided [", rows, ", ", cols, "] view");
  };
  rows16(dl, R, V, "dl");
  rows16(B, 16, V, "B");
  rows16(st, R, 16, "st");
  TORCH_CHECK(u.is_cuda() && u.is_contiguous() && u.size(0) == R && u.size(1) == 16 &&
                  u.scalar_type() == dl.scalar_type(), "lora_head_bwd: u is a contiguous [R, 16] of dl's dtype");
  TORCH_CHECK(gB.is_cuda() && gB.dim() == 2 && gB.size(0) == 16 && gB.size(1) == V &&
                  (gB.is_contiguous() || gB.t().is_contiguous()),
              "lora_head_bwd: gB is a [16, V] (transposed) contiguous block");
  const int S = bllm::lora_head_bwd_splits((int)R, (int)V, dl.stride(0));
  const int64_t slabs = (V + 1023) / 1024;
  auto gpart = at::empty({S, 16 * V}, dl.options().dtype(at::kFloat));
  auto upart = at::empty({slabs, R * 16}, dl.options().dtype(at::kFloat));
  bllm::lora_head_bwd(dt_of(dl), dl.data_ptr(), dl.stride(0), st.data_ptr(), st.stride(0), B.data_ptr(), B.stride(0),
                      gpart.data_ptr<float>(), upart.data_ptr<float>(), u.data_ptr(), (int)R, (int)V, S, stream());
  bllm::LoraWgradArgs a{};
  a.accumulate = accumulate;
  a.n = 1;
  a.r[0] = 16; a.len[0] = (int)V; a.sa[0] = gB.stride(0); a.sb[0] = gB.stride(1);
  a.gt[0][0] = gB.data_ptr();
  a.part_off[0] = 0;
  a.part = gpart.data_ptr<float>(); a.part_ld = 16 * V;
  bllm::lora_reduce(dt_of(gB), a, S, stream());
}

// dgu as swiglu_bwd, and dact is overwritten in place by act = silu(g) * u
Tensor swiglu_bwd_act(const Tensor& gu, Tensor& dact) {
  check_gpu(gu, "gu"); check_gpu(dact, "dact");
  c10::DeviceGuard g(gu.device());
  const int64_t N = gu.size(0), F = gu.size(1) / 2;
  TORCH_CHECK(dact.size(0) == N && dact.size(1) == F && dact.scalar_type() == gu.scalar_type());
  auto dgu = at::empty_like(gu);
  bllm::swiglu_bwd(dt_of(gu), gu.data_ptr(), dact.data_ptr(), dgu.data_ptr(), dact.data_ptr(), N, F, stream());
  return dgu;
}

Tensor gelu_fwd(const Tensor& f) {
  check_gpu(f, "f");
  c10::DeviceGuard g(f.device());
  auto out = at::empty_like(f);
  bllm::gelu_fwd(dt_of(f), f.data_ptr(), out.data_ptr(), f.numel(), stream());
  return out;
}

Tensor gelu_bwd(const Tensor& f, const Tensor& dg) {
  check_gpu(f, "f"); check_gpu(dg, "dg");
  c10::DeviceGuard g(f.device());
  TORCH_CHECK(f.sizes() == dg.sizes() && f.scalar_type() == dg.scalar_type());
  auto out = at::empty_like(f);
  bllm::gelu_bwd(dt_of(f), f.data_ptr(), dg.data_ptr(), out.data_ptr(), f.numel(), stream());
  return out;
}

void rope_(Tensor& qkv, const Tensor& cos, const Tensor& sin, int64_t T, int64_t H, int64_t G, int64_t hd,
           bool inverse, int64_t pos_offset) {
  check_gpu(qkv, "qkv"); check_gpu(cos, "cos"); check_gpu(sin, "sin");
  c10::DeviceGuard g(qkv.device());
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) == (H + 2 * G) * hd && hd % 2 == 0);
  TORCH_CHECK(cos.scalar_type() == at::kFloat && sin.scalar_type() == at::kFloat);
  TORCH_CHECK(cos.size(1) == hd / 2 && cos.size(0) >= T + pos_offset, "rope table too short");
  bllm::rope(dt_of(qkv), qkv.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), qkv.size(0), (int)T, (int)H,
             (int)G, (int)hd, inverse, (int)pos_offset, stream());
}

// graph-replayable RoPE of one decode token: position = pos_offset + *pos (device int32)
void rope_dev_(Tensor& qkv, const Tensor& cos, const Tensor& sin, int64_t H, int64_t G, int64_t hd,
               const Tensor& pos) {
  check_gpu(qkv, "qkv"); check_gpu(cos, "cos"); check_gpu(sin, "sin"); check_gpu(pos, "pos");
  c10::DeviceGuard g(qkv.device());
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) == (H + 2 * G) * hd && hd % 2 == 0);
  TORCH_CHECK(cos.scalar_type() == at::kFloat && sin.scalar_type() == at::kFloat && cos.size(1) == hd / 2);
  TORCH_CHECK(pos.scalar_type() == at::kInt && pos.numel() == 1, "rope_dev_: pos must be one int32");
  // T = 1: every row is one token at position *pos (the caller keeps *pos < cos.size(0))
  bllm::rope(dt_of(qkv), qkv.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), qkv.size(0), 1, (int)H,
             (int)G, (int)hd, false, 0, stream(), pos.data_ptr<int>());
}

// RoPE of a packed variable-length batch: row r at position pos_ids[r] (int32 [N])
void rope_pos_(Tensor& qkv, const Tensor& cos, const Tensor& sin, const Tensor& pos_ids, int64_t H, int64_t G,
               int64_t hd, bool inverse) {
  check_gpu(qkv, "qkv"); check_gpu(cos, "cos"); check_gpu(sin, "sin"); check_gpu(pos_ids, "pos_ids");
  c10::DeviceGuard g(qkv.device());
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) == (H + 2 * G) * hd && hd % 2 == 0 && qkv.is_contiguous(), "rope_pos_: qkv");
  TORCH_CHECK(cos.scalar_type() == at::kFloat && sin.scalar_type() == at::kFloat && cos.is_contiguous() &&
              sin.is_contiguous() && cos.dim() == 2 && cos.size(1) == hd / 2 && sin.sizes() == cos.sizes(),
              "rope_pos_: fp32 [ctx, hd/2] tables");
  TORCH_CHECK(pos_ids.scalar_type() == at::kInt && pos_ids.is_contiguous() && pos_ids.numel() == qkv.size(0),
              "rope_pos_: pos_ids must be int32 [N]");
  bllm::rope_pos(dt_of(qkv), qkv.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), pos_ids.data_ptr<int>(),
                 qkv.size(0), (int)H, (int)G, (int)hd, inverse, stream());
}

// ------------------------------------------------------------------ attention
// db (+)= dy.sum(0): dy [N, F] bf16/fp16/fp32, db [F] any float dtype (written in place)
void bias_grad_(const Tensor& dy, Tensor& db, bool accumulate) {
  check_gpu(dy, "dy"); check_gpu(db, "db");
  c10::DeviceGuard g(dy.device());
  TORCH_CHECK(dy.dim() == 2 && db.dim() == 1 && db.size(0) == dy.size(1), "bias_grad: shapes");
  const int N = (int)dy.size(0), F = (int)dy.size(1);
  TORCH_CHECK(F % (16 / (int)dy.element_size()) == 0, "bias_grad: F must be a multiple of 16 bytes");
  auto part = at::empty({bllm::colsum_bands(N, F), F}, dy.options().dtype(at::kFloat));
  bllm::bias_grad(dt_of(dy), dt_of(db), dy.data_ptr(), part.data_ptr<float>(), db.data_ptr(), N, F, accumulate,
                  stream());
}

// fused elementwise backward + bias grad: op 0 = dropout backward of src (p, seed, offset),
// op 1 = exact-GELU backward (src = dg, aux = f); returns the elementwise result, db (+)= its column sums
// db None: no bias sums; act_inplace (op 1): src is overwritten with gelu(aux)
Tensor bwd_bias_grad_(Tensor& src, const optional<Tensor>& aux, const optional<Tensor>& db_, bool accumulate,
                      int64_t op, double p, int64_t seed, int64_t offset, bool act_inplace) {
  check_gpu(src, "src");
  c10::DeviceGuard g(src.device());
  const bool has_db = db_.has_value() && db_->defined();
  TORCH_CHECK(src.dim() == 2 && src.is_contiguous(), "bwd_bias_grad: src");
  if (has_db) {
    check_gpu(*db_, "db");
    TORCH_CHECK(db_->dim() == 1 && db_->size(0) == src.size(1), "bwd_bias_grad: db shape");
  }
  TORCH_CHECK(!act_inplace || op == 1, "bwd_bias_grad: act only with the GELU backward");
  TORCH_CHECK(op == 0 || op == 1, "bwd_bias_grad: op");
  const int N = (int)src.size(0), F = (int)src.size(1);
  TORCH_CHECK(F % (16 / (int)src.element_size()) == 0, "bwd_bias_grad: F must be a multiple of 16 bytes");
  if (op == 1) {
    TORCH_CHECK(aux.has_value() && aux->sizes() == src.sizes() && aux->is_contiguous() &&
                aux->scalar_type() == src.scalar_type() && aux->device() == src.device(), "bwd_bias_grad: gelu input");
  }
  auto out = at::empty_like(src);
  Tensor part;
  if (has_db) part = at::empty({bllm::colsum_bands(N, F), F}, src.options().dtype(at::kFloat));
  bllm::bwd_bias_grad(dt_of(src), has_db ? dt_of(*db_) : dt_of(src), (int)op, src.data_ptr(),
                      op == 1 ? aux->data_ptr() : nullptr, out.data_ptr(), has_db ? part.data_ptr<float>() : nullptr,
                      has_db ? db_->data_ptr() : nullptr, N, F, accumulate, (float)p, (uint64_t)seed,
                      (uint64_t)offset, act_inplace ? src.data_ptr() : nullptr, stream());
  return out;
}

// out (+)= part.sum(0): part [S, ...] any float dtype, out contiguous with part[0]'s numel
void sum_partials_(const Tensor& part, Tensor& out, bool accumulate) {
  check_gpu(part, "part"); check_gpu(out, "out");
  c10::DeviceGuard g(part.device());
  const int64_t S = part.size(0), n = out.numel();
  TORCH_CHECK(part.numel() == S * n && n % 8 == 0, "sum_partials: shapes");
  bllm::sum_partials_into(dt_of(part), dt_of(out), part.data_ptr(), out.data_ptr(), n, (int)S, accumulate, stream());
}

// c (+)= a^T b on the token-major MFMA kernel: a [K, M], b [K, N], c [M, N], unit column
// strides, 16-B aligned rows; splits > 1 reduce K ranges into fp32 partials summed in order
void wgrad_gemm_(const Tensor& a, const Tensor& b, Tensor& c, bool accumulate, int64_t splits) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && c.is_cuda(), "wgrad_gemm: GPU tensors");
  c10::DeviceGuard g(a.device());
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && c.dim() == 2, "wgrad_gemm: 2-D operands");
  const int64_t K = a.size(0), M = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K && c.size(0) == M && c.size(1) == N, "wgrad_gemm: shapes");
  TORCH_CHECK(a.scalar_type() == b.scalar_type() &&
                  (a.scalar_type() == at::kBFloat16 || a.scalar_type() == at::kHalf), "wgrad_gemm: bf16/fp16 operands");
  TORCH_CHECK(a.stride(1) == 1 && b.stride(1) == 1 && c.stride(1) == 1, "wgrad_gemm: unit column strides");
  TORCH_CHECK(a.stride(0) % 8 == 0 && b.stride(0) % 8 == 0, "wgrad_gemm: rows must be 16-B aligned");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(a.data_ptr()) | reinterpret_cast<uintptr_t>(b.data_ptr())) % 16 == 0,
              "wgrad_gemm: operands must be 16-B aligned");
  TORCH_CHECK(a.stride(0) < (int64_t(1) << 26) && b.stride(0) < (int64_t(1) << 26), "wgrad_gemm: row stride too large");
  TORCH_CHECK(K < (int64_t(1) << 31) && M < (int64_t(1) << 31) && N < (int64_t(1) << 31));
  TORCH_CHECK(bllm::wgrad_gemm_supported((int)M, (int)N, (int)K, (int)splits), "wgrad_gemm: unsupported shape ",
              K, "x", M, "x", N, " splits ", splits);
  if (splits == 1) {
    bllm::wgrad_gemm(dt_of(a), dt_of(c), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(),
                     c.stride(0), 0, (int)M, (int)N, (int)K, 1, accumulate, stream());
    return;
  }
  TORCH_CHECK(c.is_contiguous(), "wgrad_gemm: split-K output must be contiguous");
  auto part = at::empty({splits, M, N}, a.options().dtype(at::kFloat));
  bllm::wgrad_gemm(dt_of(a), DType::F32, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), part.data_ptr(), N,
                   M * N, (int)M, (int)N, (int)K, (int)splits, false, stream());
  bllm::sum_partials_into(DType::F32, dt_of(c), part.data_ptr(), c.data_ptr(), M * N, (int)splits, accumulate,
                          stream());
}

// c (+)= a^T b with the grouped tile order in two launches: tiles [0, full) whole-K straight into c,
// the remaining tiles split St ways over K into compact fp32 partials summed into c afterwards
void wgrad_gemm_tail_(const Tensor& a, const Tensor& b, Tensor& c, bool accumulate, int64_t full, int64_t St) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && c.is_cuda(), "wgrad_gemm_tail: GPU tensors");
  c10::DeviceGuard g(a.device());
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && c.dim() == 2, "wgrad_gemm_tail: 2-D operands");
  const int64_t K = a.size(0), M = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K && c.size(0) == M && c.size(1) == N, "wgrad_gemm_tail: shapes");
  TORCH_CHECK(a.scalar_type() == b.scalar_type() &&
                  (a.scalar_type() == at::kBFloat16 || a.scalar_type() == at::kHalf), "wgrad_gemm_tail: bf16/fp16 operands");
  TORCH_CHECK(a.stride(1) == 1 && b.stride(1) == 1 && c.stride(1) == 1, "wgrad_gemm_tail: unit column strides");
  TORCH_CHECK(a.stride(0) % 8 == 0 && b.stride(0) % 8 == 0 && c.stride(0) % 8 == 0, "wgrad_gemm_tail: 16-B aligned rows");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(a.data_ptr()) | reinterpret_cast<uintptr_t>(b.data_ptr()) |
               reinterpret_cast<uintptr_t>(c.data_ptr())) % 16 == 0, "wgrad_gemm_tail: 16-B aligned operands");
  TORCH_CHECK(a.stride(0) < (int64_t(1) << 26) && b.stride(0) < (int64_t(1) << 26), "wgrad_gemm_tail: row stride too large");
  TORCH_CHECK(K < (int64_t(1) << 31) && M < (int64_t(1) << 31) && N < (int64_t(1) << 31));
  TORCH_CHECK(bllm::wgrad_tail_supported((int)M, (int)N, (int)K, (int)full, (int)St), "wgrad_gemm_tail: unsupported ",
              K, "x", M, "x", N, " full ", full, " splits ", St);
  const int64_t tail = (M / 256) * (N / 256) - full;
  auto part = at::empty({St * tail * 256 * 256}, a.options().dtype(at::kFloat));
  bllm::wgrad_gemm_tail(dt_of(a), dt_of(c), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(),
                        c.stride(0), (int)M, (int)N, (int)K, (int)full, (int)St, part.data_ptr<float>(), accumulate,
                        stream());
}

// c [M, N] (+)= a [M, K] . b [K, N], all row-major (input gradient dX = dY W of a Linear)
void gemm_nn_(const Tensor& a, const Tensor& b, Tensor& c, bool accumulate) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && c.is_cuda(), "gemm_nn: GPU tensors");
  c10::DeviceGuard g(a.device());
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && c.dim() == 2, "gemm_nn: 2-D operands");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K && c.size(0) == M && c.size(1) == N, "gemm_nn: shapes");
  TORCH_CHECK(a.scalar_type() == b.scalar_type() &&
                  (a.scalar_type() == at::kBFloat16 || a.scalar_type() == at::kHalf), "gemm_nn: bf16/fp16 operands");
  TORCH_CHECK(c.scalar_type() == a.scalar_type() || c.scalar_type() == at::kFloat, "gemm_nn: output dtype");
  TORCH_CHECK(a.stride(1) == 1 && b.stride(1) == 1 && c.stride(1) == 1, "gemm_nn: unit column strides");
  TORCH_CHECK(a.stride(0) % 8 == 0 && b.stride(0) % 8 == 0, "gemm_nn: rows must be 16-B aligned");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(a.data_ptr()) | reinterpret_cast<uintptr_t>(b.data_ptr())) % 16 == 0,
              "gemm_nn: operands must be 16-B aligned");
  TORCH_CHECK(a.stride(0) < (int64_t(1) << 26) && b.stride(0) < (int64_t(1) << 26), "gemm_nn: row stride too large");
  TORCH_CHECK(M < (int64_t(1) << 31) && N < (int64_t(1) << 31) && K < (int64_t(1) << 31));
  TORCH_CHECK(bllm::gemm_nn_supported((int)M, (int)N, (int)K), "gemm_nn: unsupported shape ", M, "x", N, "x", K);
  bllm::gemm_nn(dt_of(a), dt_of(c), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0),
                (int)M, (int)N, (int)K, accumulate, stream());
}

// c[M, N] (+)= a[M, K] . b[N, K]^T on the MFMA kernel (both operands K-contiguous)
void gemm_nt_(const Tensor& a, const Tensor& b, Tensor& c, bool accumulate) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && c.is_cuda(), "gemm_nt: GPU tensors");
  c10::DeviceGuard g(a.device());
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && c.dim() == 2, "gemm_nt: 2-D operands");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(b.size(1) == K && c.size(0) == M && c.size(1) == N, "gemm_nt: shapes");
  TORCH_CHECK(a.scalar_type() == b.scalar_type() &&
                  (a.scalar_type() == at::kBFloat16 || a.scalar_type() == at::kHalf), "gemm_nt: bf16/fp16 operands");
  TORCH_CHECK(c.scalar_type() == a.scalar_type() || c.scalar_type() == at::kFloat, "gemm_nt: output dtype");
  TORCH_CHECK(a.stride(1) == 1 && b.stride(1) == 1 && c.stride(1) == 1, "gemm_nt: unit column strides");
  TORCH_CHECK(a.stride(0) % 8 == 0 && b.stride(0) % 8 == 0, "gemm_nt: rows must be 16-B aligned");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(a.data_ptr()) | reinterpret_cast<uintptr_t>(b.data_ptr())) % 16 == 0,
              "gemm_nt: operands must be 16-B aligned");
  TORCH_CHECK(a.stride(0) < (int64_t(1) << 26) && b.stride(0) < (int64_t(1) << 26), "gemm_nt: row stride too large");
  TORCH_CHECK(M < (int64_t(1) << 31) && N < (int64_t(1) << 31) && K < (int64_t(1) << 31));
  TORCH_CHECK(bllm::gemm_nt2_supported((int)M, (int)N, (int)K, a.stride(0), b.stride(0)),
              "gemm_nt: unsupported shape ", M, "x", N, "x", K);
  bllm::gemm_nt2(dt_of(a), dt_of(c), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(),
                 c.stride(0), (int)M, (int)N, (int)K, accumulate, stream());
}

// gate/up projection + SwiGLU forward in one kernel (csrc/gemm_nt.hip): gu[M, 2F] = a . w^T with
// w = [W_gate; W_up] ([2F, K]) and act[M, F] = silu(gu[:, :F]) * gu[:, F:]
void gemm_nt_swiglu_(const Tensor& a, const Tensor& w, Tensor& gu, Tensor& act) {
  TORCH_CHECK(a.is_cuda() && w.is_cuda() && gu.is_cuda() && act.is_cuda(), "gemm_nt_swiglu: GPU tensors");
  c10::DeviceGuard g(a.device());
  TORCH_CHECK(a.dim() == 2 && w.dim() == 2 && gu.dim() == 2 && act.dim() == 2, "gemm_nt_swiglu: 2-D operands");
  const int64_t M = a.size(0), K = a.size(1), F = w.size(0) / 2;
  TORCH_CHECK(w.size(0) == 2 * F && w.size(1) == K && gu.size(0) == M && gu.size(1) == 2 * F && act.size(0) == M &&
                  act.size(1) == F && act.is_contiguous(), "gemm_nt_swiglu: shapes");
  TORCH_CHECK(a.scalar_type() == w.scalar_type() && gu.scalar_type() == a.scalar_type() &&
                  act.scalar_type() == a.scalar_type() &&
                  (a.scalar_type() == at::kBFloat16 || a.scalar_type() == at::kHalf), "gemm_nt_swiglu: bf16/fp16");
  TORCH_CHECK(a.stride(1) == 1 && w.stride(1) == 1 && gu.stride(1) == 1, "gemm_nt_swiglu: unit column strides");
  TORCH_CHECK(a.stride(0) % 8 == 0 && w.stride(0) % 8 == 0 && gu.stride(0) % 8 == 0, "gemm_nt_swiglu: 16-B rows");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(a.data_ptr()) | reinterpret_cast<uintptr_t>(w.data_ptr()) |
               reinterpret_cast<uintptr_t>(gu.data_ptr()) | reinterpret_cast<uintptr_t>(act.data_ptr())) % 16 == 0,
              "gemm_nt_swiglu: 16-B aligned operands");
  TORCH_CHECK(bllm::gemm_nt_swiglu_supported((int)M, (int)F, (int)K, a.stride(0), w.stride(0), gu.stride(0)),
              "gemm_nt_swiglu: unsupported shape ", M, "x", F, "x", K);
  bllm::gemm_nt_swiglu(dt_of(a), a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), gu.data_ptr(), gu.stride(0),
                       act.data_ptr(), (int)M, (int)F, (int)K, stream());
}

// QKV projection with RoPE in the epilogue (K4, csrc/gemm_nt.hip): qkv[M, N] = a . w^T, columns
// below nrot rotated at position row % T (tables fp32 [>= T, 64], head dim 128)
void gemm_nt_rope_(const Tensor& a, const Tensor& w, Tensor& qkv, const Tensor& cos, const Tensor& sin, int64_t T,
                   int64_t nrot, int64_t hd) {
  TORCH_CHECK(a.is_cuda() && w.is_cuda() && qkv.is_cuda() && cos.is_cuda() && sin.is_cuda(), "gemm_nt_rope: GPU tensors");
  c10::DeviceGuard g(a.device());
  TORCH_CHECK(a.dim() == 2 && w.dim() == 2 && qkv.dim() == 2, "gemm_nt_rope: 2-D operands");
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && qkv.size(0) == M && qkv.size(1) == N, "gemm_nt_rope: shapes");
  TORCH_CHECK(a.scalar_type() == w.scalar_type() && qkv.scalar_type() == a.scalar_type() &&
                  (a.scalar_type() == at::kBFloat16 || a.scalar_type() == at::kHalf), "gemm_nt_rope: bf16/fp16");
  TORCH_CHECK(cos.scalar_type() == at::kFloat && sin.scalar_type() == at::kFloat && cos.is_contiguous() &&
                  sin.is_contiguous() && cos.size(1) == hd / 2 && sin.sizes() == cos.sizes() && cos.size(0) >= T,
              "gemm_nt_rope: fp32 [>= T, hd/2] tables");
  TORCH_CHECK(a.stride(1) == 1 && w.stride(1) == 1 && qkv.stride(1) == 1 && a.stride(0) % 8 == 0 &&
                  w.stride(0) % 8 == 0, "gemm_nt_rope: unit column strides, 16-B rows");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(a.data_ptr()) | reinterpret_cast<uintptr_t>(w.data_ptr())) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 8 == 0, "gemm_nt_rope: aligned operands");
  TORCH_CHECK(nrot % hd == 0 && nrot <= N && T > 0, "gemm_nt_rope: nrot");
  TORCH_CHECK(bllm::gemm_nt_rope_supported((int)M, (int)N, (int)K, a.stride(0), w.stride(0), qkv.stride(0), (int)hd),
              "gemm_nt_rope: unsupported shape ", M, "x", N, "x", K, " hd ", hd);
  bllm::gemm_nt_rope(dt_of(a), a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), qkv.data_ptr(), qkv.stride(0),
                     (int)M, (int)N, (int)K, cos.data_ptr<float>(), sin.data_ptr<float>(), (int)T, (int)nrot, stream());
}

// GPT-2 c_fc with bias + exact GELU in the epilogue (K9, csrc/gemm_nt.hip): f = a . w^T + bias,
// g = gelu(f); f and g contiguous [M, N]
void gemm_nt_bias_gelu_(const Tensor& a, const Tensor& w, const Tensor& bias, Tensor& f, Tensor& g) {
  TORCH_CHECK(a.is_cuda() && w.is_cuda() && bias.is_cuda() && f.is_cuda() && g.is_cuda(), "gemm_nt_bias_gelu: GPU");
  c10::DeviceGuard dg(a.device());
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(a.dim() == 2 && w.dim() == 2 && w.size(1) == K && bias.numel() == N && bias.is_contiguous() &&
                  f.sizes() == g.sizes() && f.size(0) == M && f.size(1) == N && f.is_contiguous() && g.is_contiguous(),
              "gemm_nt_bias_gelu: shapes");
  TORCH_CHECK(a.scalar_type() == w.scalar_type() && bias.scalar_type() == a.scalar_type() &&
                  f.scalar_type() == a.scalar_type() && g.scalar_type() == a.scalar_type() &&
                  (a.scalar_type() == at::kBFloat16 || a.scalar_type() == at::kHalf), "gemm_nt_bias_gelu: bf16/fp16");
  TORCH_CHECK(a.stride(1) == 1 && w.stride(1) == 1 && a.stride(0) % 8 == 0 && w.stride(0) % 8 == 0 &&
                  (reinterpret_cast<uintptr_t>(a.data_ptr()) | reinterpret_cast<uintptr_t>(w.data_ptr())) % 16 == 0 &&
                  (reinterpret_cast<uintptr_t>(bias.data_ptr()) | reinterpret_cast<uintptr_t>(f.data_ptr()) |
                   reinterpret_cast<uintptr_t>(g.data_ptr())) % 8 == 0, "gemm_nt_bias_gelu: alignment");
  TORCH_CHECK(bllm::gemm_nt_bias_gelu_supported((int)M, (int)N, (int)K, a.stride(0), w.stride(0), f.stride(0)),
              "gemm_nt_bias_gelu: unsupported shape ", M, "x", N, "x", K);
  bllm::gemm_nt_bias_gelu(dt_of(a), a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), bias.data_ptr(),
                          f.data_ptr(), g.data_ptr(), f.stride(0), (int)M, (int)N, (int)K, stream());
}

// qkv [B, (H+2G)*hd] (one decode token per row); kc / vc [B, G, Tmax, hd] valid below *pos;
// appends the token's k / v at *pos and attends over pos + 1 keys -> out [B, H*hd]
Tensor attn_decode_append(const Tensor& qkv, Tensor& kc, Tensor& vc, const Tensor& pos, int64_t H, int64_t G) {
  check_gpu(qkv, "qkv"); check_gpu(kc, "kcache"); check_gpu(vc, "vcache"); check_gpu(pos, "pos");
  c10::DeviceGuard g(qkv.device());
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 || qkv.scalar_type() == at::kHalf, "attn_decode_append: bf16/fp16");
  TORCH_CHECK(kc.scalar_type() == qkv.scalar_type() && vc.scalar_type() == qkv.scalar_type());
  TORCH_CHECK(kc.dim() == 4 && vc.sizes() == kc.sizes() && kc.is_contiguous() && vc.is_contiguous());
  TORCH_CHECK(qkv.dim() == 2 && qkv.is_contiguous() && H % G == 0 && kc.size(1) == G, "attn_decode_append: shapes");
  const int64_t B = qkv.size(0), hd = kc.size(3), Tmax = kc.size(2);
  TORCH_CHECK(qkv.size(1) == (H + 2 * G) * hd && kc.size(0) == B, "attn_decode_append: qkv / cache mismatch");
  TORCH_CHECK(hd == 64 || hd == 128, "attn_decode_append: head_dim 64 or 128");
  TORCH_CHECK(Tmax <= bllm::attn_decode_max_len(), "attn_decode_append: cache longer than the LDS score buffer");
  TORCH_CHECK(pos.scalar_type() == at::kInt && pos.numel() == 1, "attn_decode_append: pos must be one int32");
  auto out = at::empty({B, H * hd}, qkv.options());
  bllm::attn_decode_append(dt_of(qkv), qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                           pos.data_ptr<int>(), (int)B, (int)H, (int)G, (int)hd, (int)Tmax, stream());
  return out;
}

// q [B, H, hd]; kc / vc [B, G, Tmax, hd] with the first L positions valid -> out [B, H*hd]
Tensor attn_decode(const Tensor& q, const Tensor& kc, const Tensor& vc, int64_t L) {
  check_gpu(q, "q"); check_gpu(kc, "kcache"); check_gpu(vc, "vcache");
  c10::DeviceGuard g(q.device());
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 || q.scalar_type() == at::kHalf, "attn_decode: bf16/fp16 only");
  TORCH_CHECK(kc.scalar_type() == q.scalar_type() && vc.scalar_type() == q.scalar_type());
  TORCH_CHECK(q.dim() == 3 && kc.dim() == 4 && vc.sizes() == kc.sizes(), "attn_decode: shapes");
  const int64_t B = q.size(0), H = q.size(1), hd = q.size(2), G = kc.size(1), Tmax = kc.size(2);
  TORCH_CHECK(kc.size(0) == B && kc.size(3) == hd && H % G == 0, "attn_decode: cache/q mismatch");
  TORCH_CHECK(hd == 64 || hd == 128, "attn_decode: head_dim 64 or 128");
  TORCH_CHECK(L >= 1 && L <= Tmax && L <= bllm::attn_decode_max_len(), "attn_decode: bad length ", L);
  auto out = at::empty({B, H * hd}, q.options());
  bllm::attn_decode(dt_of(q), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), (int)B, (int)H, (int)G,
                    (int)hd, (int)Tmax, (int)L, stream());
  return out;
}

// keep_mask: optional uint32 [B*H, ceil(T/32), T] the forward fills with the dropout keep bits
// (dropout > 0, bf16/fp16) and the backward reads (api.h attn_fwd)
static uint32_t* keep_mask_ptr(const optional<Tensor>& m, const Tensor& qkv, int64_t B, int64_t T, int64_t H,
                               int64_t hd, double p) {
  if (!m.has_value() || p <= 0.0 || !bllm::attn_keep_mask_ok(dt_of(qkv), (int)hd)) return nullptr;
  check_gpu(*m, "keep_mask");
  TORCH_CHECK(m->scalar_type() == at::kInt && m->numel() == B * H * ((T + 31) / 32) * T,
              "flash_attn: keep_mask must be int32 [B*H, ceil(T/32), T]");
  return reinterpret_cast<uint32_t*>(m->data_ptr<int32_t>());
}

std::tuple<Tensor, Tensor> flash_attn_fwd(const Tensor& qkv, int64_t B, int64_t T, int64_t H, int64_t G,
                                          int64_t hd, bool causal, double p, int64_t seed, int64_t offset,
                                          const optional<Tensor>& keep_mask) {
  check_gpu(qkv, "qkv");
  c10::DeviceGuard g(qkv.device());
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 || qkv.scalar_type() == at::kHalf ||
              qkv.scalar_type() == at::kFloat, "flash_attn: bf16/fp16/fp32 only");
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) == B * T && qkv.size(1) == (H + 2 * G) * hd);
  TORCH_CHECK(H % G == 0, "flash_attn: n_heads must be a multiple of n_kv_groups");
  TORCH_CHECK(bllm::attn_supported_head_dim((int)hd), "flash_attn: unsupported head_dim ", hd);
  auto o = at::empty({B * T, H * hd}, qkv.options());
  auto lse = at::empty({B, H, T}, qkv.options().dtype(at::kFloat));
  bllm::attn_fwd(dt_of(qkv), qkv.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), (int)B, (int)T, (int)H, (int)G,
                 (int)hd, causal, (float)p, (uint64_t)seed, (uint64_t)offset,
                 keep_mask_ptr(keep_mask, qkv, B, T, H, hd, p), stream());
  return {o, lse};
}

// fp32 [>= T, hd/2] RoPE table for the inverse rotation fused into the attention backward
static const float* rope_ptr(const optional<Tensor>& t, const Tensor& qkv, int64_t T, int64_t hd) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->device() == qkv.device() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->dim() == 2 &&
              t->size(0) >= T && t->size(1) == hd / 2, "flash_attn_bwd: rope table must be fp32 [>= T, hd/2] on the qkv device");
  return t->data_ptr<float>();
}

// placement experiments / tests: tile maps of the dW and forward-layout GEMM kernels
void set_gemm_tile_maps(int64_t wg_map, int64_t wg_gm, int64_t nt_map, int64_t nt_gm) {
  bllm::set_wgrad_tile_map((int)wg_map, (int)wg_gm);
  bllm::set_gemm_nt_tile_map((int)nt_map, (int)nt_gm);
}

Tensor flash_attn_bwd(const Tensor& qkv, const Tensor& o, const Tensor& lse, const Tensor& dout, int64_t B,
                      int64_t T, int64_t H, int64_t G, int64_t hd, bool causal, double p, int64_t seed,
                      int64_t offset, const optional<Tensor>& keep_mask, const optional<Tensor>& rope_cos,
                      const optional<Tensor>& rope_sin) {
  check_gpu(qkv, "qkv"); check_gpu(o, "o"); check_gpu(lse, "lse"); check_gpu(dout, "dout");
  c10::DeviceGuard g(qkv.device());
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 || qkv.scalar_type() == at::kHalf ||
              qkv.scalar_type() == at::kFloat);
  TORCH_CHECK(o.scalar_type() == qkv.scalar_type() && dout.scalar_type() == qkv.scalar_type(), "flash_attn_bwd: dtypes");
  TORCH_CHECK(qkv.is_contiguous() && o.is_contiguous() && dout.is_contiguous(), "flash_attn_bwd: contiguous inputs");
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) == B * T && qkv.size(1) == (H + 2 * G) * hd);
  TORCH_CHECK(o.sizes() == dout.sizes() && o.size(0) == B * T && o.size(1) == H * hd);
  TORCH_CHECK(bllm::attn_supported_head_dim((int)hd), "flash_attn: unsupported head_dim ", hd);
  auto dqkv = at::empty_like(qkv);
  auto delta = at::empty({B, H, T}, qkv.options().dtype(at::kFloat));
  const bool mfma = qkv.scalar_type() != at::kFloat && bllm::attn_mfma_head_dim((int)hd);
  // per-query-head dK/dV partials only for GQA (MHA writes dK/dV directly); dQ is atomic-free
  auto dkv_part = (mfma && bllm::attn_bwd_kv_partials((int)B, (int)T, (int)H, (int)G)) ? at::empty({2, B * T, H, hd}, qkv.options().dtype(at::kFloat)) : Tensor();
  bllm::attn_bwd(dt_of(qkv), qkv.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), dout.data_ptr(), dqkv.data_ptr(),
                 delta.data_ptr<float>(), dkv_part.defined() ? dkv_part.data_ptr<float>() : nullptr, (int)B, (int)T, (int)H, (int)G, (int)hd, causal,
                 (float)p, (uint64_t)seed, (uint64_t)offset, keep_mask_ptr(keep_mask, qkv, B, T, H, hd, p),
                 rope_ptr(rope_cos, qkv, T, hd), rope_ptr(rope_sin, qkv, T, hd), stream());
  return dqkv;
}

// Variable-length attention (causal, no dropout) on a packed batch: sequence b is rows
// [cu[b], cu[b+1]) of qkv [N, (H+2G) hd]; bf16 / fp16, head dims 64 / 128 (the matrix-core kernels)
static void check_varlen(const Tensor& qkv, const Tensor& cu, int64_t max_len, int64_t H, int64_t G, int64_t hd) {
  check_gpu(qkv, "qkv"); check_gpu(cu, "cu");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 || qkv.scalar_type() == at::kHalf, "flash_attn_varlen: bf16/fp16 only");
  TORCH_CHECK(hd == 64 || hd == 128, "flash_attn_varlen: head_dim 64 or 128, got ", hd);
  TORCH_CHECK(G > 0 && H % G == 0, "flash_attn_varlen: n_heads must be a multiple of n_kv_groups");
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) == (H + 2 * G) * hd && qkv.is_contiguous(), "flash_attn_varlen: qkv");
  TORCH_CHECK(cu.scalar_type() == at::kInt && cu.is_contiguous() && cu.dim() == 1 && cu.numel() >= 1 &&
              cu.device() == qkv.device(), "flash_attn_varlen: cu must be int32 [B + 1] on the qkv device");
  TORCH_CHECK(max_len >= 0 && max_len <= qkv.size(0), "flash_attn_varlen: max_len");
}

std::tuple<Tensor, Tensor> flash_attn_varlen_fwd(const Tensor& qkv, const Tensor& cu, int64_t max_len, int64_t H,
                                                 int64_t G, int64_t hd) {
  check_varlen(qkv, cu, max_len, H, G, hd);
  c10::DeviceGuard g(qkv.device());
  const int64_t N = qkv.size(0), B = cu.numel() - 1;
  auto o = at::empty({N, H * hd}, qkv.options());
  auto lse = at::empty({H * N}, qkv.options().dtype(at::kFloat));
  bllm::attn_fwd_mfma_varlen(dt_of(qkv), qkv.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), cu.data_ptr<int>(),
                             (int)B, (int)max_len, (int)H, (int)G, (int)hd, stream());
  return {o, lse};
}

Tensor flash_attn_varlen_bwd(const Tensor& qkv, const Tensor& o, const Tensor& lse, const Tensor& dout,
                             const Tensor& cu, const Tensor& pos_ids, int64_t max_len, int64_t H, int64_t G,
                             int64_t hd, const optional<Tensor>& rope_cos, const optional<Tensor>& rope_sin) {
  check_varlen(qkv, cu, max_len, H, G, hd);
  check_gpu(o, "o"); check_gpu(lse, "lse"); check_gpu(dout, "dout"); check_gpu(pos_ids, "pos_ids");
  c10::DeviceGuard g(qkv.device());
  const int64_t N = qkv.size(0), B = cu.numel() - 1;
  TORCH_CHECK(o.scalar_type() == qkv.scalar_type() && dout.scalar_type() == qkv.scalar_type(), "flash_attn_varlen_bwd: dtypes");
  TORCH_CHECK(o.is_contiguous() && dout.is_contiguous() && lse.is_contiguous(), "flash_attn_varlen_bwd: contiguous inputs");
  TORCH_CHECK(o.sizes() == dout.sizes() && o.dim() == 2 && o.size(0) == N && o.size(1) == H * hd, "flash_attn_varlen_bwd: o / dout");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == H * N, "flash_attn_varlen_bwd: lse must be fp32 [H * N]");
  TORCH_CHECK(pos_ids.scalar_type() == at::kInt && pos_ids.is_contiguous() && pos_ids.numel() == N,
              "flash_attn_varlen_bwd: pos_ids must be int32 [N]");
  auto dqkv = at::empty_like(qkv);
  auto delta = at::empty({H * N}, qkv.options().dtype(at::kFloat));
  auto dkv_part = bllm::attn_bwd_kv_partials((int)B, (int)max_len, (int)H, (int)G)
                      ? at::empty({2, N, H, hd}, qkv.options().dtype(at::kFloat)) : Tensor();
  bllm::attn_bwd_mfma_varlen(dt_of(qkv), qkv.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), dout.data_ptr(),
                             dqkv.data_ptr(), delta.data_ptr<float>(),
                             dkv_part.defined() ? dkv_part.data_ptr<float>() : nullptr, cu.data_ptr<int>(),
                             pos_ids.data_ptr<int>(), N, (int)B, (int)max_len, (int)H, (int)G, (int)hd,
                             rope_ptr(rope_cos, qkv, max_len, hd), rope_ptr(rope_sin, qkv, max_len, hd), stream());
  return dqkv;
}

// ------------------------------------------------------------------ loss
// logits may be a row-strided view (unit stride within a row): the vocabulary padded to whole
// GEMM tiles in the fused head, CE over the first V columns
static void check_logits(const Tensor& logits) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1 && logits.stride(0) >= logits.size(1),
              "bllm ce: logits must be a 2-D GPU tensor with unit-stride rows");
}

std::tuple<Tensor, Tensor> ce_fwd(const Tensor& logits, const Tensor& targets, int64_t ignore_index) {
  check_logits(logits); check_gpu(targets, "targets");
  c10::DeviceGuard g(logits.device());
  TORCH_CHECK(targets.dim() == 1 && targets.size(0) == logits.size(0));
  TORCH_CHECK(targets.scalar_type() == at::kLong);
  const int64_t N = logits.size(0), V = logits.size(1);
  auto loss = at::empty({N}, logits.options().dtype(at::kFloat));
  auto lse = at::empty({N}, logits.options().dtype(at::kFloat));
  bllm::ce_fwd(dt_of(logits), logits.data_ptr(), targets.data_ptr<int64_t>(), loss.data_ptr<float>(),
               lse.data_ptr<float>(), N, V, logits.stride(0), ignore_index, stream());
  return {loss, lse};
}

void ce_bwd_(Tensor& logits, const Tensor& targets, const Tensor& lse, const Tensor& scale, int64_t ignore_index) {
  check_logits(logits); check_gpu(targets, "targets"); check_gpu(lse, "lse"); check_gpu(scale, "scale");
  c10::DeviceGuard g(logits.device());
  TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.numel() >= 1);
  const int64_t N = logits.size(0), V = logits.size(1);
  bllm::ce_bwd(dt_of(logits), logits.data_ptr(), targets.data_ptr<int64_t>(), lse.data_ptr<float>(),
               scale.data_ptr<float>(), N, V, logits.stride(0), ignore_index, stream());
}

// ------------------------------------------------------------------ embedding
Tensor embedding_fwd(const Tensor& idx, const Tensor& wte, const optional<Tensor>& wpe, int64_t T, double p,
                     int64_t seed, int64_t offset) {
  check_gpu(idx, "idx"); check_gpu(wte, "wte");
  c10::DeviceGuard g(wte.device());
  TORCH_CHECK(idx.scalar_type() == at::kLong);
  const int64_t N = idx.numel(), d = wte.size(1);
  const void* pe = nullptr;
  if (wpe.has_value()) {
    check_gpu(*wpe, "wpe");
    TORCH_CHECK(wpe->size(1) == d && wpe->size(0) >= T && N % T == 0);
    pe = wpe->data_ptr();
  }
  auto out = at::empty({N, d}, wte.options());
  bllm::embedding_fwd(dt_of(wte), idx.data_ptr<int64_t>(), wte.data_ptr(), pe, out.data_ptr(), N, (int)d, (int)T,
                      (float)p, (uint64_t)seed, (uint64_t)offset, (long)wte.size(0), stream());
  return out;
}

void embedding_bwd(const Tensor& idx, const Tensor& dx, const optional<Tensor>& grad_wte,
                   const optional<Tensor>& grad_wpe, int64_t T, bool accumulate) {
  check_gpu(idx, "idx"); check_gpu(dx, "dx");
  c10::DeviceGuard g(dx.device());
  const int64_t N = idx.numel(), d = dx.size(1);
  if (grad_wte.has_value()) {
    Tensor gw = *grad_wte;
    check_gpu(gw, "grad_wte");
    TORCH_CHECK(gw.size(1) == d && gw.scalar_type() == dx.scalar_type());
    if (!accumulate) gw.zero_();
    // stable: equal ids keep their token order, so the fp32 sums run in a fixed order
    auto sorted = at::sort(idx.reshape({-1}), /*stable=*/true, 0, false);
    Tensor sid = std::get<0>(sorted).contiguous(), perm = std::get<1>(sorted).contiguous();
    auto part = at::empty({bllm::embedding_bwd_part_floats(N, (int)d)}, dx.options().dtype(at::kFloat));
    bllm::embedding_bwd_tok(dt_of(dx), sid.data_ptr<int64_t>(), perm.data_ptr<int64_t>(), dx.data_ptr(),
                            gw.data_ptr(), part.data_ptr<float>(), N, (int)d, accumulate, stream());
  }
  if (grad_wpe.has_value()) {
    Tensor gp = *grad_wpe;
    check_gpu(gp, "grad_wpe");
    TORCH_CHECK(N % T == 0 && gp.size(1) == d && gp.size(0) >= T);
    if (!accumulate && gp.size(0) > T) gp.zero_();
    bllm::embedding_bwd_pos(dt_of(dx), dx.data_ptr(), gp.data_ptr(), (int)(N / T), (int)T, (int)d, accumulate,
                            stream());
  }
}

// ------------------------------------------------------------------ LoRA (csrc/lora.hip)
static void check_lora_mat(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 2, "bllm lora: ", name, " must be a 2-D GPU tensor");
  TORCH_CHECK(t.stride(1) == 1 && t.stride(0) % 8 == 0 && (uintptr_t)t.data_ptr() % 16 == 0,
              "bllm lora: ", name, " rows must be 16-byte aligned and unit-stride");
}

// out[:, ocol_i : ocol_i + r_i] = scale * x[:, c0_i : c0_i + len_i] . w_i^T ;  w_i [r_i, >= len_i]
static void lora_down_impl(const Tensor& x, at::TensorList ws, at::IntArrayRef c0, at::IntArrayRef lens,
                           at::IntArrayRef ocol, int64_t R, double scale, Tensor& out) {
  check_lora_mat(x, "x");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, "lora_down: bf16/fp16 only");
  const int64_t N = x.size(0);
  TORCH_CHECK(N > 0 && R % 16 == 0 && R > 0, "lora_down: N > 0 and R a multiple of 16 required");
  TORCH_CHECK(ws.size() == c0.size() && ws.size() == lens.size() && ws.size() == ocol.size());
  TORCH_CHECK(out.is_cuda() && out.dim() == 2 && out.size(0) == N && out.size(1) >= R && out.stride(1) == 1 &&
                  out.scalar_type() == x.scalar_type(), "lora_down: out must be an [N, >= R] row-strided view");
  bllm::LoraDownArgs a{};
  a.x = x.data_ptr(); a.ldx = x.stride(0); a.out = out.data_ptr(); a.ldo = out.stride(0); a.scale = (float)scale;
  a.R = (int)R; a.zpad = (int)(out.size(1) - R);  // columns past R: zeros (alignment pad)
  for (size_t i = 0; i < ws.size(); ++i) {
    const Tensor& w = ws[i];
    check_lora_mat(w, "w");
    TORCH_CHECK(w.scalar_type() == x.scalar_type(), "lora_down: dtype mismatch");
    const int64_t r = w.size(0);
    TORCH_CHECK(r % 16 == 0 && lens[i] % 32 == 0 && c0[i] % 8 == 0 && w.size(1) >= lens[i],
                "lora_down: rank % 16, len % 32, c0 % 8 required");
    TORCH_CHECK(c0[i] + lens[i] <= x.size(1) && ocol[i] + r <= R && ocol[i] % 8 == 0, "lora_down: window out of range");
    for (int64_t off = 0; off < r; off += 64) {
      TORCH_CHECK(a.n < bllm::LORA_MAX, "lora_down: too many rank chunks");
      a.c0[a.n] = (int)c0[i]; a.len[a.n] = (int)lens[i]; a.ocol[a.n] = (int)(ocol[i] + off);
      a.nt[a.n] = (int)(std::min<int64_t>(64, r - off) / 16);
      a.w[a.n] = (const char*)w.data_ptr() + off * w.stride(0) * w.element_size();
      a.ldw[a.n] = w.stride(0);
      ++a.n;
    }
  }
  bllm::lora_down(dt_of(x), a, (int)N, stream());
}

Tensor lora_down(const Tensor& x, at::TensorList ws, at::IntArrayRef c0, at::IntArrayRef lens,
                 at::IntArrayRef ocol, int64_t R, double scale) {
  auto out = at::empty({x.size(0), R}, x.options());
  lora_down_impl(x, ws, c0, lens, ocol, R, scale, out);
  return out;
}

// dst [rows, R] (any strides, one of them 1): member i's B_i^T [len_i, r_i] at rows c0_i.., columns
// off_i.., zeros elsewhere -- the B block of a K-augmented LoRA weight, one launch per group
void lora_block_(Tensor& dst, at::TensorList bs, at::IntArrayRef c0, at::IntArrayRef off) {
  TORCH_CHECK(dst.is_cuda() && dst.dim() == 2 && (dst.stride(0) == 1 || dst.stride(1) == 1) &&
                  (dst.scalar_type() == at::kBFloat16 || dst.scalar_type() == at::kHalf), "lora_block_: dst");
  c10::DeviceGuard g(dst.device());
  TORCH_CHECK(bs.size() == c0.size() && bs.size() == off.size() && (int64_t)bs.size() <= bllm::LORA_MAX);
  bllm::LoraBlockArgs a{};
  a.dst = dst.data_ptr(); a.s_row = dst.stride(0); a.s_j = dst.stride(1);
  a.rows = (int)dst.size(0); a.R = (int)dst.size(1); a.n = (int)bs.size();
  for (size_t i = 0; i < bs.size(); ++i) {
    const Tensor& b = bs[i];
    TORCH_CHECK(b.is_cuda() && b.dim() == 2 && b.stride(1) == 1 && b.scalar_type() == dst.scalar_type(),
                "lora_block_: B must be a row-major [r, len] GPU tensor of dst's dtype");
    TORCH_CHECK(c0[i] + b.size(1) <= dst.size(0) && off[i] + b.size(0) <= dst.size(1), "lora_block_: block out of range");
    a.c0[i] = (int)c0[i]; a.len[i] = (int)b.size(1); a.off[i] = (int)off[i]; a.r[i] = (int)b.size(0);
    a.b[i] = b.data_ptr(); a.ldb[i] = b.stride(0);
  }
  bllm::lora_block(dt_of(dst), a, stream());
}

// writes into a row-strided view, e.g. the s t columns of a K-augmented [x | s t] operand
void lora_down_into_(const Tensor& x, at::TensorList ws, at::IntArrayRef c0, at::IntArrayRef lens,
                     at::IntArrayRef ocol, int64_t R, double scale, Tensor& out) {
  lora_down_impl(x, ws, c0, lens, ocol, R, scale, out);
}

// y[:, c0_i : c0_i + len_i] = base + bias + scale * t[:, toff_i : toff_i + r_i] . u_i ;  u_i [r_i, len_i], any
// strides; base (same shape as y, may be y itself) and bias ([y.size(1)]) are optional
void lora_up_(Tensor& y, const Tensor& t, at::TensorList us, at::IntArrayRef c0, at::IntArrayRef toff, double scale,
              const optional<Tensor>& base, const optional<Tensor>& bias) {
  check_lora_mat(y, "y"); check_lora_mat(t, "t");
  c10::DeviceGuard g(y.device());
  TORCH_CHECK(y.scalar_type() == t.scalar_type() && (y.scalar_type() == at::kBFloat16 || y.scalar_type() == at::kHalf));
  const int64_t N = y.size(0);
  TORCH_CHECK(t.size(0) == N && N > 0, "lora_up: t rows must match y");
  TORCH_CHECK(us.size() == c0.size() && us.size() == toff.size() && (int)us.size() <= bllm::LORA_MAX);
  bllm::LoraUpArgs a{};
  a.y = y.data_ptr(); a.ldy = y.stride(0); a.t = t.data_ptr(); a.ldt = t.stride(0); a.scale = (float)scale;
  if (base.has_value()) {
    check_lora_mat(*base, "base");
    TORCH_CHECK(base->sizes() == y.sizes() && base->scalar_type() == y.scalar_type(), "lora_up: base shape");
    a.base = base->data_ptr(); a.ldb = base->stride(0);
  }
  if (bias.has_value()) {
    check_gpu(*bias, "bias");
    TORCH_CHECK(bias->numel() == y.size(1) && bias->scalar_type() == y.scalar_type() &&
                (uintptr_t)bias->data_ptr() % 16 == 0, "lora_up: bias");
    a.bias = bias->data_ptr();
  }
  int max_len = 0;
  for (size_t i = 0; i < us.size(); ++i) {
    const Tensor& u = us[i];
    TORCH_CHECK(u.is_cuda() && u.dim() == 2 && u.scalar_type() == y.scalar_type(), "lora_up: u must be 2-D");
    const int64_t r = u.size(0), len = u.size(1);
    TORCH_CHECK(r % 16 == 0 && r <= 256 && toff[i] % 8 == 0 && toff[i] + r <= t.size(1), "lora_up: rank window");
    TORCH_CHECK(c0[i] % 8 == 0 && len % 8 == 0 && c0[i] + len <= y.size(1), "lora_up: output window");
    a.c0[a.n] = (int)c0[i]; a.len[a.n] = (int)len; a.toff[a.n] = (int)toff[i]; a.r[a.n] = (int)r;
    a.u[a.n] = u.data_ptr(); a.su_j[a.n] = u.stride(0); a.su_c[a.n] = u.stride(1);
    max_len = std::max<int>(max_len, (int)len);
    ++a.n;
  }
  bllm::lora_up(dt_of(y), a, (int)N, max_len, stream());
}

// g_i[a][b] (+)= scale * sum_n p[n][pa_i + a] * q[n][qb_i + b] ;  g_i [r_i, len_i] view of a contiguous block
void lora_wgrad(const Tensor& p, const Tensor& q, at::TensorList gs, at::IntArrayRef pa, at::IntArrayRef qb,
                double scale, bool accumulate) {
  check_lora_mat(p, "p"); check_lora_mat(q, "q");
  c10::DeviceGuard g(p.device());
  TORCH_CHECK(p.scalar_type() == q.scalar_type() && (p.scalar_type() == at::kBFloat16 || p.scalar_type() == at::kHalf));
  const int64_t N = p.size(0);
  TORCH_CHECK(q.size(0) == N && N > 0, "lora_wgrad: p / q token counts differ");
  TORCH_CHECK(gs.size() == pa.size() && gs.size() == qb.size() && (int)gs.size() <= bllm::LORA_MAX && !gs.empty());
  bllm::LoraWgradArgs a{};
  a.p = p.data_ptr(); a.ldp = p.stride(0); a.q = q.data_ptr(); a.ldq = q.stride(0);
  a.scale = (float)scale; a.accumulate = accumulate;
  const DType odt = dt_of(gs[0]);
  const int64_t esz = gs[0].element_size();
  int blocks = 0;
  for (size_t i = 0; i < gs.size(); ++i) {
    const Tensor& gm = gs[i];
    TORCH_CHECK(gm.is_cuda() && gm.dim() == 2 && dt_of(gm) == odt, "lora_wgrad: grads must share a dtype");
    TORCH_CHECK(gm.is_contiguous() || gm.t().is_contiguous(), "lora_wgrad: grad must be a (transposed) contiguous block");
    const int64_t r = gm.size(0), len = gm.size(1);
    TORCH_CHECK(r % 16 == 0 && r <= 64 && len % 8 == 0 && pa[i] % 8 == 0 && qb[i] % 8 == 0, "lora_wgrad: alignment");
    TORCH_CHECK(pa[i] + r <= p.size(1) && qb[i] + len <= q.size(1), "lora_wgrad: window out of range");
    // merge into the previous member when both read the same Q window, their P windows are
    // adjacent, their output strides agree and the merged rank stays <= 64 (dA of a group)
    if (a.n > 0) {
      const int j = a.n - 1;
      if (a.qb[j] == (int)qb[i] && a.len[j] == (int)len && a.pa[j] + a.r[j] == (int)pa[i] && a.r[j] + r <= 64 &&
          a.sa[j] == gm.stride(0) && a.sb[j] == gm.stride(1)) {
        for (int64_t t = 0; t < r / 16; ++t)
          a.gt[j][a.r[j] / 16 + t] = (char*)gm.data_ptr() + 16 * t * gm.stride(0) * esz;
        a.r[j] += (int)r;
        continue;
      }
    }
    a.pa[a.n] = (int)pa[i]; a.qb[a.n] = (int)qb[i]; a.r[a.n] = (int)r; a.len[a.n] = (int)len;
    a.nblk[a.n] = bllm::ceil_div(len, 64); a.sa[a.n] = gm.stride(0); a.sb[a.n] = gm.stride(1);
    for (int64_t t = 0; t < r / 16; ++t) a.gt[a.n][t] = (char*)gm.data_ptr() + 16 * t * gm.stride(0) * esz;
    ++a.n;
  }
  for (int i = 0; i < a.n; ++i) blocks += a.nblk[i];
  const int S = bllm::lora_wgrad_splits(blocks, (int)N);
  Tensor part;
  if (S > 1) {
    int64_t total = 0;
    for (int i = 0; i < a.n; ++i) { a.part_off[i] = total; total += (int64_t)a.len[i] * a.r[i]; }
    part = at::empty({S, total}, p.options().dtype(at::kFloat));
    a.part = part.data_ptr<float>(); a.part_ld = total;
  }
  bllm::lora_wgrad(dt_of(p), odt, a, (int)N, S, stream());
}

// [R, K] = concat_i a_i^T  (a_i [K, r_i] contiguous)
Tensor lora_pack_t(at::TensorList as) {
  TORCH_CHECK(!as.empty() && (int)as.size() <= bllm::LORA_MAX);
  c10::DeviceGuard g(as[0].device());
  const int64_t K = as[0].size(0);
  bllm::LoraPackArgs a{};
  int64_t R = 0;
  int max_r = 0;
  for (auto& t : as) {
    check_gpu(t, "lora A");
    TORCH_CHECK(t.dim() == 2 && t.size(0) == K && t.scalar_type() == as[0].scalar_type());
    a.off[a.n] = (int)R; a.r[a.n] = (int)t.size(1); a.a[a.n] = t.data_ptr();
    R += t.size(1);
    max_r = std::max<int>(max_r, (int)t.size(1));
    ++a.n;
  }
  auto out = at::empty({R, K}, as[0].options());
  a.out = out.data_ptr();
  bllm::lora_pack_t(dt_of(as[0]), a, (int)K, max_r, stream());
  return out;
}

// ------------------------------------------------------------------ optimizer
Tensor sq_norm_multi(at::TensorList ts) {
  TORCH_CHECK(!ts.empty());
  c10::DeviceGuard g(ts[0].device());
  std::vector<int> slots;
  int total = 0;
  for (auto& t : ts) {
    check_gpu(t, "tensor");
    slots.push_back(bllm::sqsum_slots(t.numel()));
    total += slots.back();
  }
  auto part = at::empty({total}, ts[0].options().dtype(at::kFloat));
  auto out = at::empty({1}, ts[0].options().dtype(at::kFloat));
  int off = 0;
  for (size_t i = 0; i < ts.size(); ++i) {
    bllm::sqsum_partial(dt_of(ts[i]), ts[i].data_ptr(), ts[i].numel(), part.data_ptr<float>() + off, slots[i],
                        stream());
    off += slots[i];
  }
  bllm::sum_partials(part.data_ptr<float>(), total, out.data_ptr<float>(), stream());
  return out;
}

void adamw_step_(Tensor& param, const optional<Tensor>& master, const Tensor& grad, Tensor& exp_avg,
                 Tensor& exp_avg_sq, double lr, double b1, double b2, double eps, double wd, int64_t step,
                 const optional<Tensor>& grad_scale) {
  check_gpu(param, "param"); check_gpu(grad, "grad"); check_gpu(exp_avg, "exp_avg"); check_gpu(exp_avg_sq, "exp_avg_sq");
  c10::DeviceGuard g(param.device());
  const int64_t n = param.numel();
  TORCH_CHECK(grad.numel() == n && exp_avg.numel() == n && exp_avg_sq.numel() == n);
  TORCH_CHECK(exp_avg.scalar_type() == at::kFloat && exp_avg_sq.scalar_type() == at::kFloat);
  float* mp = nullptr;
  if (master.has_value()) {
    check_gpu(*master, "master");
    TORCH_CHECK(master->numel() == n && master->scalar_type() == at::kFloat);
    mp = master->data_ptr<float>();
  }
  const float* gs = nullptr;
  if (grad_scale.has_value()) {
    check_gpu(*grad_scale, "grad_scale");
    TORCH_CHECK(grad_scale->scalar_type() == at::kFloat);
    gs = grad_scale->data_ptr<float>();
  }
  bllm::adamw_step(dt_of(param), dt_of(grad), param.data_ptr(), mp, grad.data_ptr(), exp_avg.data_ptr<float>(),
                   exp_avg_sq.data_ptr<float>(), n, lr, b1, b2, eps, wd, (int)step, gs, stream());
}

}  // namespace


// ----------------------------------------------------------------------------- residual GEMM
// D[N, O] = x[N, K] @ W[O, K]^T + C[N, O] as ONE hipBLASLt matmul with C != D.  torch.addmm with
// a 2-D `self` first copies C into the output and then runs a beta=1 GEMM in place (a 200 MB
// copy kernel per o/down projection at Llama-3-8B B=24, profiles/r1_llama3_8b_1gpu_v7.md); here
// the GEMM reads C in its epilogue.  Column-major view: D^T (O x N) = op_T(W: K x O) * x^T (K x N),
// the same TN family torch picks for nn.Linear.  Heuristic top-1 solution, cached per shape.
#define LT_CHECK(x)                                                                  \
  do {                                                                               \
    hipblasStatus_t st_ = (x);                                                       \
    TORCH_CHECK(st_ == HIPBLAS_STATUS_SUCCESS, "hipBLASLt: ", #x, " failed (", (int)st_, ")"); \
  } while (0)

namespace {
constexpr size_t kLtWorkspace = 64ull << 20;
struct LtPlan {
  hipblasLtMatmulDesc_t op = nullptr;
  hipblasLtMatrixLayout_t a = nullptr, b = nullptr, c = nullptr;
  hipblasLtMatmulAlgo_t algo;
};
std::mutex lt_mu;
hipblasLtHandle_t lt_handle(int dev) {
  static hipblasLtHandle_t h[64] = {};
  std::lock_guard<std::mutex> g(lt_mu);
  if (!h[dev]) LT_CHECK(hipblasLtCreate(&h[dev]));
  return h[dev];
}
const LtPlan& lt_plan(int dev, hipDataType dt, int64_t N, int64_t K, int64_t O) {
  static std::map<std::tuple<int, int, int64_t, int64_t, int64_t>, LtPlan> cache;
  const auto key = std::make_tuple(dev, (int)dt, N, K, O);
  {
    std::lock_guard<std::mutex> g(lt_mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
  }
  hipblasLtHandle_t h = lt_handle(dev);
  LtPlan p;
  LT_CHECK(hipblasLtMatmulDescCreate(&p.op, HIPBLAS_COMPUTE_32F, HIP_R_32F));
  hipblasOperation_t ta = HIPBLAS_OP_T, tb = HIPBLAS_OP_N;
  LT_CHECK(hipblasLtMatmulDescSetAttribute(p.op, HIPBLASLT_MATMUL_DESC_TRANSA, &ta, sizeof(ta)));
  LT_CHECK(hipblasLtMatmulDescSetAttribute(p.op, HIPBLASLT_MATMUL_DESC_TRANSB, &tb, sizeof(tb)));
  LT_CHECK(hipblasLtMatrixLayoutCreate(&p.a, dt, K, O, K));  // W [O, K] row-major
  LT_CHECK(hipblasLtMatrixLayoutCreate(&p.b, dt, K, N, K));  // x [N, K] row-major
  LT_CHECK(hipblasLtMatrixLayoutCreate(&p.c, dt, O, N, O));  // C, D [N, O] row-major
  hipblasLtMatmulPreference_t pref;
  LT_CHECK(hipblasLtMatmulPreferenceCreate(&pref));
  uint64_t ws = kLtWorkspace;
  LT_CHECK(hipblasLtMatmulPreferenceSetAttribute(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &ws, sizeof(ws)));
  // heuristic top-1: timing the top 16 on the real operands measured 0.4 % slower end to end
  // (profiles/r5/lt_tune/) and made the choice process-dependent; removed in round 5
  hipblasLtMatmulHeuristicResult_t res[1];
  int n = 0;
  LT_CHECK(hipblasLtMatmulAlgoGetHeuristic(h, p.op, p.a, p.b, p.c, p.c, pref, 1, res, &n));
  hipblasLtMatmulPreferenceDestroy(pref);
  TORCH_CHECK(n > 0, "hipBLASLt: no solution for residual GEMM N=", N, " K=", K, " O=", O);
  p.algo = res[0].algo;
  std::lock_guard<std::mutex> g(lt_mu);
  return cache.emplace(key, p).first->second;
}
}  // namespace

Tensor linear_residual(const Tensor& x, const Tensor& W, const Tensor& C) {
  check_gpu(x, "x"); check_gpu(W, "W"); check_gpu(C, "C");
  TORCH_CHECK(x.dim() == 2 && W.dim() == 2 && C.dim() == 2, "linear_residual: 2-D operands");
  TORCH_CHECK(x.is_contiguous() && W.is_contiguous() && C.is_contiguous(), "linear_residual: contiguous operands");
  TORCH_CHECK(x.scalar_type() == W.scalar_type() && x.scalar_type() == C.scalar_type(), "linear_residual: one dtype");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, "linear_residual: bf16/fp16");
  const int64_t N = x.size(0), K = x.size(1), O = W.size(0);
  TORCH_CHECK(W.size(1) == K && C.size(0) == N && C.size(1) == O, "linear_residual: shape mismatch");
  c10::DeviceGuard g(x.device());
  const int dev = x.get_device();
  TORCH_CHECK(dev >= 0 && dev < 64);
  const hipDataType dt = x.scalar_type() == at::kBFloat16 ? HIP_R_16BF : HIP_R_16F;
  auto D = at::empty({N, O}, x.options());
  auto ws = at::empty({(int64_t)kLtWorkspace}, x.options().dtype(at::kByte));
  const LtPlan& p = lt_plan(dev, dt, N, K, O);
  const float alpha = 1.f, beta = 1.f;
  LT_CHECK(hipblasLtMatmul(lt_handle(dev), p.op, &alpha, W.data_ptr(), p.a, x.data_ptr(), p.b, &beta, C.data_ptr(),
                           p.c, D.data_ptr(), p.c, &p.algo, ws.data_ptr(), kLtWorkspace, stream()));
  return D;
}

// ------------------------------------------------------------------ kernel debug mode
// First failed device-side check since the last call (common.h DebugCode; 0 = none), over every
// instrumented translation unit; always 0 in release builds (the checks are compiled away).
int64_t debug_error() {
  const unsigned codes[] = {bllm::debug_take_embedding(), bllm::debug_take_loss(), bllm::debug_take_attn_decode(),
                            bllm::debug_take_elementwise()};
  for (unsigned c : codes)
    if (c) return (int64_t)c;
  return 0;
}
bool kernel_debug_build() {
#ifdef BLLM_KERNEL_DEBUG
  return true;
#else
  return false;
#endif
}

TORCH_LIBRARY(bllm, m) {
  m.def("debug_error() -> int", &debug_error);
  m.def("set_gemm_tile_maps(int wg_map, int wg_gm, int nt_map, int nt_gm) -> ()", &set_gemm_tile_maps);
  m.def("kernel_debug_build() -> bool", &kernel_debug_build);
  m.def("rmsnorm_fwd(Tensor x, Tensor w, float eps) -> (Tensor, Tensor)");
  m.def("rmsnorm_fwd_into_(Tensor x, Tensor w, float eps, Tensor(a!) y) -> Tensor");
  m.def("rmsnorm_bwd(Tensor dy, Tensor x, Tensor w, Tensor rstd, Tensor? dx_acc, Tensor(a!)? dw_out, bool accumulate) -> (Tensor, Tensor)");
  m.def("layernorm_fwd(Tensor x, Tensor w, Tensor b, float eps) -> (Tensor, Tensor, Tensor)");
  m.def("layernorm_bwd(Tensor dy, Tensor x, Tensor w, Tensor mean, Tensor rstd, Tensor? dx_acc, Tensor(a!)? dw_out, Tensor(b!)? db_out, bool accumulate) -> (Tensor, Tensor, Tensor)");
  m.def("dropout_add(Tensor x, Tensor a, float p, int seed, int offset) -> Tensor");
  m.def("dropout_add_layernorm(Tensor x, Tensor a, Tensor w, Tensor b, float eps, float p, int seed, int offset) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("dropout_bwd(Tensor dy, float p, int seed, int offset) -> Tensor");
  m.def("bwd_bias_grad_(Tensor(a!) src, Tensor? aux, Tensor(b!)? db, bool accumulate, int op, float p, int seed, int offset, bool act_inplace=False) -> Tensor");
  m.def("transpose2d(Tensor a) -> Tensor");
  m.def("linear_residual(Tensor x, Tensor W, Tensor C) -> Tensor");
  m.def("swiglu_fwd(Tensor gu) -> Tensor");
  m.def("swiglu_fwd_into_(Tensor gu, Tensor(a!) act) -> ()");
  m.def("swiglu_bwd_lowrank(Tensor gu, Tensor base, Tensor u, Tensor P, float scale) -> Tensor");
  m.def("swiglu_bwd_lowrank_wgrad(Tensor gu, Tensor base, Tensor u, Tensor P, float scale, Tensor st, Tensor(a!) gB_gate, Tensor(b!) gB_up, Tensor(c!) gA_down_t, bool accumulate) -> Tensor");
  m.def("lora_head_bwd_(Tensor dl, Tensor st, Tensor B, Tensor(a!) u, Tensor(b!) gB, bool accumulate) -> ()");
  m.def("swiglu_bwd(Tensor gu, Tensor dact) -> Tensor");
  m.def("swiglu_bwd_act(Tensor gu, Tensor(a!) dact) -> Tensor");
  m.def("gelu_fwd(Tensor f) -> Tensor");
  m.def("gelu_bwd(Tensor f, Tensor dg) -> Tensor");
  m.def("rope_(Tensor(a!) qkv, Tensor cos, Tensor sin, int T, int H, int G, int hd, bool inverse, int pos_offset) -> ()");
  m.def("bias_grad_(Tensor dy, Tensor(a!) db, bool accumulate) -> ()");
  m.def("sum_partials_(Tensor part, Tensor(a!) out, bool accumulate) -> ()");
  m.def("wgrad_gemm_(Tensor a, Tensor b, Tensor(a!) c, bool accumulate, int splits) -> ()");
  m.def("wgrad_gemm_tail_(Tensor a, Tensor b, Tensor(a!) c, bool accumulate, int full, int St) -> ()");
  m.def("gemm_nn_(Tensor a, Tensor b, Tensor(a!) c, bool accumulate) -> ()");
  m.def("gemm_nt_(Tensor a, Tensor b, Tensor(a!) c, bool accumulate) -> ()");
  m.def("gemm_nt_swiglu_(Tensor a, Tensor w, Tensor(a!) gu, Tensor(b!) act) -> ()");
  m.def("gemm_nt_rope_(Tensor a, Tensor w, Tensor(a!) qkv, Tensor cos, Tensor sin, int T, int nrot, int hd) -> ()");
  m.def("gemm_nt_bias_gelu_(Tensor a, Tensor w, Tensor bias, Tensor(a!) f, Tensor(b!) g) -> ()");
  m.def("attn_decode(Tensor q, Tensor kcache, Tensor vcache, int L) -> Tensor");
  m.def("attn_decode_append(Tensor qkv, Tensor(a!) kcache, Tensor(b!) vcache, Tensor pos, int H, int G) -> Tensor");
  m.def("rope_dev_(Tensor(a!) qkv, Tensor cos, Tensor sin, int H, int G, int hd, Tensor pos) -> ()");
  m.def("rope_pos_(Tensor(a!) qkv, Tensor cos, Tensor sin, Tensor pos_ids, int H, int G, int hd, bool inverse) -> ()");
  m.def("flash_attn_varlen_fwd(Tensor qkv, Tensor cu, int max_len, int H, int G, int hd) -> (Tensor, Tensor)");
  m.def("flash_attn_varlen_bwd(Tensor qkv, Tensor o, Tensor lse, Tensor dout, Tensor cu, Tensor pos_ids, int max_len, int H, int G, int hd, Tensor? rope_cos=None, Tensor? rope_sin=None) -> Tensor");
  m.def("flash_attn_fwd(Tensor qkv, int B, int T, int H, int G, int hd, bool causal, float p, int seed, int offset, Tensor(a!)? keep_mask=None) -> (Tensor, Tensor)");
  m.def("flash_attn_bwd(Tensor qkv, Tensor o, Tensor lse, Tensor dout, int B, int T, int H, int G, int hd, bool causal, float p, int seed, int offset, Tensor? keep_mask=None, Tensor? rope_cos=None, Tensor? rope_sin=None) -> Tensor");
  m.def("ce_fwd(Tensor logits, Tensor targets, int ignore_index) -> (Tensor, Tensor)");
  m.def("ce_bwd_(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor scale, int ignore_index) -> ()");
  m.def("embedding_fwd(Tensor idx, Tensor wte, Tensor? wpe, int T, float p, int seed, int offset) -> Tensor");
  m.def("embedding_bwd(Tensor idx, Tensor dx, Tensor(a!)? grad_wte, Tensor(b!)? grad_wpe, int T, bool accumulate) -> ()");
  m.def("lora_down(Tensor x, Tensor[] ws, int[] c0, int[] lens, int[] ocol, int R, float scale) -> Tensor");
  m.def("lora_block_(Tensor(a!) dst, Tensor[] bs, int[] c0, int[] off) -> ()");
  m.def("lora_down_into_(Tensor x, Tensor[] ws, int[] c0, int[] lens, int[] ocol, int R, float scale, Tensor(a!) out) -> ()");
  m.def("lora_up_(Tensor(a!) y, Tensor t, Tensor[] us, int[] c0, int[] toff, float scale, Tensor? base, Tensor? bias) -> ()");
  m.def("lora_wgrad(Tensor p, Tensor q, Tensor(a!)[] gs, int[] pa, int[] qb, float scale, bool accumulate) -> ()");
  m.def("lora_pack_t(Tensor[] a) -> Tensor");
  m.def("sq_norm_multi(Tensor[] ts) -> Tensor");
  m.def("adamw_step_(Tensor(a!) param, Tensor(b!)? master, Tensor grad, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, float lr, float beta1, float beta2, float eps, float wd, int step, Tensor? grad_scale) -> ()");
}

TORCH_LIBRARY_IMPL(bllm, CUDA, m) {
  m.impl("rmsnorm_fwd", &rmsnorm_fwd);
  m.impl("rmsnorm_fwd_into_", &rmsnorm_fwd_into_);
  m.impl("rmsnorm_bwd", &rmsnorm_bwd);
  m.impl("layernorm_fwd", &layernorm_fwd);
  m.impl("layernorm_bwd", &layernorm_bwd);
  m.impl("dropout_add", &dropout_add);
  m.impl("dropout_add_layernorm", &dropout_add_layernorm);
  m.impl("dropout_bwd", &dropout_bwd);
  m.impl("bwd_bias_grad_", &bwd_bias_grad_);
  m.impl("transpose2d", &transpose2d);
  m.impl("linear_residual", &linear_residual);
  m.impl("swiglu_fwd", &swiglu_fwd);
  m.impl("swiglu_fwd_into_", &swiglu_fwd_into_);
  m.impl("swiglu_bwd_lowrank", &swiglu_bwd_lowrank);
  m.impl("swiglu_bwd_lowrank_wgrad", &swiglu_bwd_lowrank_wgrad);
  m.impl("lora_head_bwd_", &lora_head_bwd_);
  m.impl("swiglu_bwd", &swiglu_bwd);
  m.impl("swiglu_bwd_act", &swiglu_bwd_act);
  m.impl("gelu_fwd", &gelu_fwd);
  m.impl("gelu_bwd", &gelu_bwd);
  m.impl("rope_", &rope_);
  m.impl("flash_attn_fwd", &flash_attn_fwd);
  m.impl("attn_decode", &attn_decode);
  m.impl("attn_decode_append", &attn_decode_append);
  m.impl("rope_dev_", &rope_dev_);
  m.impl("sum_partials_", &sum_partials_);
  m.impl("wgrad_gemm_", &wgrad_gemm_);
  m.impl("wgrad_gemm_tail_", &wgrad_gemm_tail_);
  m.impl("gemm_nn_", &gemm_nn_);
  m.impl("gemm_nt_", &gemm_nt_);
  m.impl("gemm_nt_swiglu_", &gemm_nt_swiglu_);
  m.impl("gemm_nt_rope_", &gemm_nt_rope_);
  m.impl("gemm_nt_bias_gelu_", &gemm_nt_bias_gelu_);
  m.impl("bias_grad_", &bias_grad_);
  m.impl("flash_attn_bwd", &flash_attn_bwd);
  m.impl("rope_pos_", &rope_pos_);
  m.impl("flash_attn_varlen_fwd", &flash_attn_varlen_fwd);
  m.impl("flash_attn_varlen_bwd", &flash_attn_varlen_bwd);
  m.impl("ce_fwd", &ce_fwd);
  m.impl("ce_bwd_", &ce_bwd_);
  m.impl("embedding_fwd", &embedding_fwd);
  m.impl("embedding_bwd", &embedding_bwd);
  m.impl("lora_down", &lora_down);
  m.impl("lora_down_into_", &lora_down_into_);
  m.impl("lora_block_", &lora_block_);
  m.impl("lora_up_", &lora_up_);
  m.impl("lora_wgrad", &lora_wgrad);
  m.impl("lora_pack_t", &lora_pack_t);
  m.impl("sq_norm_multi", &sq_norm_multi);
  m.impl("adamw_step_", &adamw_step_);
}
