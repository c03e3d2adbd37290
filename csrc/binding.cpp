// torch.ops.bllm.* registration for the gfx950 kernel library.
//
// Before a launch, every pointer the launcher receives is known to cover what the kernel reads
// and writes through it, in the dtype the kernel assumes, on one GPU (a bad launch on the shared
// GPU pool can reset the node).  Each op states that with the small check vocabulary below; every
// message starts with the op name and names the argument, and is formatted only on failure.
// Values that live in device memory (token ids, cu, *pos) are the kernel-debug build's business.
// Ops allocate outputs through the PyTorch HIP caching allocator and launch on the current HIP
// stream, so they compose with torch streams, events and hipGraph capture.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>
#include <hipblaslt/hipblaslt.h>

#include <algorithm>
#include <climits>
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

// ------------------------------------------------------------------ argument checks
bool is_half(const Tensor& t) { return t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf; }
bool aligned(const Tensor& t, int64_t bytes) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0; }

// optional tensor -> the tensor or nullptr, and that -> its data pointer, or nullptr when absent / undefined
const Tensor* opt(const optional<Tensor>& o) { return o.has_value() && o->defined() ? &*o : nullptr; }
template <typename T = void>
T* opt_ptr(const Tensor* t) { return t && t->defined() ? static_cast<T*>(t->data_ptr()) : nullptr; }

// One op call: its name (the start of every message), the GPU of its first tensor, where every
// other tensor must live too, and the device guard for the allocations and launches.
struct Op {
  const char* name;
  c10::Device dev;
  c10::DeviceGuard guard;
  Op(const char* n, const Tensor& x, const char* what) : name(n), dev(x.device()), guard(dev) {
    TORCH_CHECK(x.is_cuda(), n, ": ", what, " must be a GPU tensor");
  }

  void on_gpu(const Tensor& t, const char* what) const {
    TORCH_CHECK(t.device() == dev, name, ": ", what, " must be on ", dev, ", got ", t.device());
  }
  void contig(const Tensor& t, const char* what) const {
    on_gpu(t, what);
    TORCH_CHECK(t.is_contiguous(), name, ": ", what, " must be contiguous");
  }
  void dims(const Tensor& t, int64_t n, const char* what) const {
    TORCH_CHECK(t.dim() == n, name, ": ", what, " must be ", n, "-D, got ", t.sizes());
  }
  void dtype(const Tensor& t, at::ScalarType dt, const char* what) const {
    TORCH_CHECK(t.scalar_type() == dt, name, ": ", what, " must be ", dt, ", got ", t.scalar_type());
  }
  void floating(const Tensor& t, const char* what) const {
    TORCH_CHECK(is_half(t) || t.scalar_type() == at::kFloat, name, ": ", what, " must be bf16, fp16 or fp32");
  }
  // contiguous bf16 / fp16 / fp32 tensor
  void dense(const Tensor& t, const char* what) const {
    floating(t, what);
    contig(t, what);
  }
  void half_only(const Tensor& t, const char* what) const {
    TORCH_CHECK(is_half(t), name, ": ", what, " must be bf16 or fp16, got ", t.scalar_type());
  }
  // an int64 that goes into an int parameter of api.h
  int to_int(int64_t v, const char* what = "a size or index") const {
    TORCH_CHECK(v >= INT_MIN && v <= INT_MAX, name, ": ", what, " = ", v, " does not fit an int");
    return (int)v;
  }
  // contiguous tensor of this dtype with exactly n elements
  void vec(const Tensor& t, int64_t n, at::ScalarType dt, const char* what) const {
    contig(t, what);
    dtype(t, dt, what);
    TORCH_CHECK(t.numel() == n, name, ": ", what, " must have ", n, " elements, got ", t.numel());
  }
  // contiguous tensor of this shape (a negative size: any) and dtype
  void shaped(const Tensor& t, at::IntArrayRef shape, at::ScalarType dt, const char* what) const {
    contig(t, what);
    dtype(t, dt, what);
    bool ok = t.dim() == (int64_t)shape.size();
    for (size_t i = 0; ok && i < shape.size(); ++i) ok = shape[i] < 0 || t.size(i) == shape[i];
    TORCH_CHECK(ok, name, ": ", what, " must have shape ", shape, ", got ", t.sizes());
  }
  void like(const Tensor& t, const Tensor& ref, const char* what) const {
    shaped(t, ref.sizes(), ref.scalar_type(), what);
  }
  // [nr, nc] view (a negative size: any; at_least: nc or more columns) of this dtype with unit
  // column stride and rows that do not overlap; base and row pitch multiples of `align` bytes, by
  // default the 16 B of the kernels' vector loads and stores
  void rows(const Tensor& t, int64_t nr, int64_t nc, at::ScalarType dt, const char* what, bool at_least = false,
            int64_t align = 16) const {
    on_gpu(t, what);
    dtype(t, dt, what);
    const bool shape_ok = t.dim() == 2 && (nr < 0 || t.size(0) == nr) &&
                          (nc < 0 || t.size(1) == nc || (at_least && t.size(1) > nc));
    TORCH_CHECK(shape_ok, name, ": ", what, " must be [", nr, at_least ? ", >= " : ", ", nc, "], got ", t.sizes());
    TORCH_CHECK(t.stride(1) == 1 && (t.size(0) <= 1 || t.stride(0) >= t.size(1)) &&
                    (t.stride(0) * t.element_size()) % align == 0 && aligned(t, align),
                name, ": ", what, " must be a row-strided view with unit column stride and ", align,
                "-byte aligned rows, got strides ", t.strides());
  }
  // [rows, cols] gradient block of any float dtype, contiguous or the transpose of a contiguous [cols, rows]
  void grad_block(const Tensor& t, int64_t rows, int64_t cols, const char* what) const {
    on_gpu(t, what);
    floating(t, what);
    TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == cols &&
                    ((t.stride(0) == cols && t.stride(1) == 1) || (t.stride(0) == 1 && t.stride(1) == rows)),
                name, ": ", what, " must be a [", rows, ", ", cols, "] (transposed) contiguous block, got ", t.sizes(),
                " strides ", t.strides());
  }
};

// ------------------------------------------------------------------ norms
// x [N, d]: contiguous rows of whole 16-B vectors, no longer than the kernels' register budget; w [d] of x's dtype
std::pair<int, int> norm_rows(const Op& op, const Tensor& x, const Tensor& w) {
  op.dense(x, "x");
  TORCH_CHECK(x.dim() == 2 && x.size(1) % (16 / x.element_size()) == 0 && x.size(1) <= bllm::norm_max_dim(dt_of(x)),
              op.name, ": x must be [N, d] with d a multiple of ", 16 / x.element_size(), " and at most ",
              bllm::norm_max_dim(dt_of(x)), ", got ", x.sizes());
  op.vec(w, x.size(1), x.scalar_type(), "w");
  return {op.to_int(x.size(0), "N"), op.to_int(x.size(1), "d")};
}

// y: a [N, d] row-strided view (stride(0) >= d, 16-B aligned rows), e.g. the x part of a
// K-augmented LoRA operand [x | s t]; returns rstd
Tensor rmsnorm_into(const char* name, const Tensor& x, const Tensor& w, double eps, Tensor& y) {
  Op op(name, x, "x");
  const auto [N, d] = norm_rows(op, x, w);
  op.rows(y, N, d, x.scalar_type(), "y");
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  bllm::rmsnorm_fwd(dt_of(x), x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr<float>(), N, d, (float)eps,
                    (long)y.stride(0), stream());
  return rstd;
}
Tensor rmsnorm_fwd_into_(const Tensor& x, const Tensor& w, double eps, Tensor& y) {
  return rmsnorm_into("rmsnorm_fwd_into_", x, w, eps, y);
}
std::tuple<Tensor, Tensor> rmsnorm_fwd(const Tensor& x, const Tensor& w, double eps) {
  auto y = at::empty_like(x);
  return {y, rmsnorm_into("rmsnorm_fwd", x, w, eps, y)};
}

// dW goes to `dw_out` (any float dtype, written or accumulated) when given, else a new fp32 [d]
Tensor grad_vec(const Op& op, const optional<Tensor>& o, const Tensor& x, int64_t d, const char* what) {
  if (!o.has_value()) return at::empty({d}, x.options().dtype(at::kFloat));
  op.floating(*o, what);
  op.vec(*o, d, o->scalar_type(), what);
  return *o;
}

std::tuple<Tensor, Tensor> rmsnorm_bwd(const Tensor& dy, const Tensor& x, const Tensor& w, const Tensor& rstd,
                                       const optional<Tensor>& dx_acc, const optional<Tensor>& dw_out,
                                       bool accumulate) {
  Op op("rmsnorm_bwd", x, "x");
  const auto [N, d] = norm_rows(op, x, w);
  op.like(dy, x, "dy");
  op.vec(rstd, N, at::kFloat, "rstd");
  const Tensor* acc = opt(dx_acc);
  if (acc) op.like(*acc, x, "dx_acc");
  auto dx = at::empty_like(x);
  const int nwg = bllm::norm_bwd_num_wg(N, d);
  auto part = at::empty({nwg, d}, x.options().dtype(at::kFloat));
  Tensor dw = grad_vec(op, dw_out, x, d, "dw_out");
  bllm::rmsnorm_bwd(dt_of(x), dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr<float>(), opt_ptr(acc),
                    dx.data_ptr(), part.data_ptr<float>(), dt_of(dw), dw.data_ptr(), accumulate && dw_out.has_value(),
                    N, d, nwg, stream());
  return {dx, dw};
}

std::tuple<Tensor, Tensor, Tensor> layernorm_fwd(const Tensor& x, const Tensor& w, const Tensor& b, double eps) {
  Op op("layernorm_fwd", x, "x");
  const auto [N, d] = norm_rows(op, x, w);
  op.vec(b, d, x.scalar_type(), "b");
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
  Op op("layernorm_bwd", x, "x");
  const auto [N, d] = norm_rows(op, x, w);
  op.like(dy, x, "dy");
  op.vec(mean, N, at::kFloat, "mean");
  op.vec(rstd, N, at::kFloat, "rstd");
  const Tensor* acc = opt(dx_acc);
  if (acc) op.like(*acc, x, "dx_acc");
  auto dx = at::empty_like(x);
  const int nwg = bllm::norm_bwd_num_wg(N, d);
  auto pw = at::empty({nwg, d}, x.options().dtype(at::kFloat));
  auto pb = at::empty({nwg, d}, x.options().dtype(at::kFloat));
  TORCH_CHECK(dw_out.has_value() == db_out.has_value(), "layernorm_bwd: give both dw_out and db_out or neither");
  Tensor dw = grad_vec(op, dw_out, x, d, "dw_out");
  Tensor db = grad_vec(op, db_out, x, d, "db_out");
  TORCH_CHECK(dw.scalar_type() == db.scalar_type(), "layernorm_bwd: dw_out / db_out dtypes differ");
  bllm::layernorm_bwd(dt_of(x), dy.data_ptr(), x.data_ptr(), w.data_ptr(), mean.data_ptr<float>(),
                      rstd.data_ptr<float>(), opt_ptr(acc), dx.data_ptr(), pw.data_ptr<float>(), pb.data_ptr<float>(),
                      dt_of(dw), dw.data_ptr(), db.data_ptr(), accumulate && dw_out.has_value(), N, d, nwg,
                      stream());
  return {dx, dw, db};
}

// x2 = x + dropout(a), (y, mean, rstd) = LayerNorm(x2): one pass (GPT-2's attention residual + norm2)
std::tuple<Tensor, Tensor, Tensor, Tensor> dropout_add_layernorm(const Tensor& x, const Tensor& a, const Tensor& w,
                                                                 const Tensor& b, double eps, double p, int64_t seed,
                                                                 int64_t offset) {
  Op op("dropout_add_layernorm", x, "x");
  const auto [N, d] = norm_rows(op, x, w);
  op.like(a, x, "a");
  op.vec(b, d, x.scalar_type(), "b");
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
  Op op("dropout_add", x, "x");
  op.dense(x, "x");
  op.like(a, x, "a");
  auto out = at::empty_like(x);
  bllm::dropout_add(dt_of(x), x.data_ptr(), a.data_ptr(), out.data_ptr(), x.numel(), (float)p, (uint64_t)seed,
                    (uint64_t)offset, stream());
  return out;
}

Tensor dropout_bwd(const Tensor& dy, double p, int64_t seed, int64_t offset) {
  Op op("dropout_bwd", dy, "dy");
  op.dense(dy, "dy");
  auto out = at::empty_like(dy);
  bllm::dropout_add(dt_of(dy), nullptr, dy.data_ptr(), out.data_ptr(), dy.numel(), (float)p, (uint64_t)seed,
                    (uint64_t)offset, stream());
  return out;
}

Tensor transpose2d(const Tensor& a) {
  Op op("transpose2d", a, "a");
  op.contig(a, "a");
  TORCH_CHECK(a.dim() == 2 && a.element_size() == 2, "transpose2d: a must be a 2-D 16-bit tensor");
  const int64_t R = a.size(0), C = a.size(1);
  TORCH_CHECK(R % 8 == 0 && C % 8 == 0, "transpose2d: both dims must be multiples of 8, got ", a.sizes());
  auto out = at::empty({C, R}, a.options());
  bllm::transpose16(a.data_ptr(), out.data_ptr(), R, C, stream());
  return out;
}

Tensor gelu_fwd(const Tensor& f) {
  Op op("gelu_fwd", f, "f");
  op.dense(f, "f");
  auto out = at::empty_like(f);
  bllm::gelu_fwd(dt_of(f), f.data_ptr(), out.data_ptr(), f.numel(), stream());
  return out;
}

Tensor gelu_bwd(const Tensor& f, const Tensor& dg) {
  Op op("gelu_bwd", f, "f");
  op.dense(f, "f");
  op.like(dg, f, "dg");
  auto out = at::empty_like(f);
  bllm::gelu_bwd(dt_of(f), f.data_ptr(), dg.data_ptr(), out.data_ptr(), f.numel(), stream());
  return out;
}

// gu [N, 2F] = [gate | up], contiguous -> {N, F}
std::pair<int64_t, int> swiglu_dims(const Op& op, const Tensor& gu) {
  op.dense(gu, "gu");
  TORCH_CHECK(gu.dim() == 2 && gu.size(1) % 2 == 0, op.name, ": gu must be [N, 2F], got ", gu.sizes());
  return {gu.size(0), op.to_int(gu.size(1) / 2, "F")};
}

// act: a [N, F] row-strided view (the act part of a K-augmented [act | s t] operand)
void swiglu_into(const char* name, const Tensor& gu, Tensor& act, int64_t align) {
  Op op(name, gu, "gu");
  const auto [N, F] = swiglu_dims(op, gu);
  op.rows(act, N, F, gu.scalar_type(), "act", false, align);
  bllm::swiglu_fwd(dt_of(gu), gu.data_ptr(), act.data_ptr(), N, F, (long)act.stride(0), stream());
}
void swiglu_fwd_into_(const Tensor& gu, Tensor& act) { swiglu_into("swiglu_fwd_into_", gu, act, 16); }
Tensor swiglu_fwd(const Tensor& gu) {
  TORCH_CHECK(gu.dim() == 2, "swiglu_fwd: gu must be [N, 2F], got ", gu.sizes());
  auto act = at::empty({gu.size(0), gu.size(1) / 2}, gu.options());
  swiglu_into("swiglu_fwd", gu, act, gu.element_size());  // odd F: the scalar kernel, no alignment needed
  return act;
}

// dgu from dact [N, F]; write_act: dact is overwritten in place by act = silu(g) * u
Tensor swiglu_bwd_impl(const char* name, const Tensor& gu, const Tensor& dact, bool write_act) {
  Op op(name, gu, "gu");
  const auto [N, F] = swiglu_dims(op, gu);
  op.shaped(dact, {N, F}, gu.scalar_type(), "dact");
  auto dgu = at::empty_like(gu);
  bllm::swiglu_bwd(dt_of(gu), gu.data_ptr(), dact.data_ptr(), dgu.data_ptr(), write_act ? dact.data_ptr() : nullptr, N,
                   F, stream());
  return dgu;
}
Tensor swiglu_bwd(const Tensor& gu, const Tensor& dact) { return swiglu_bwd_impl("swiglu_bwd", gu, dact, false); }
Tensor swiglu_bwd_act(const Tensor& gu, Tensor& dact) { return swiglu_bwd_impl("swiglu_bwd_act", gu, dact, true); }

// swiglu_bwd with dact = base + scale . u P (base [N, F] and u [N, r] row-strided views, P [r, F])
Tensor swiglu_bwd_lowrank(const Tensor& gu, const Tensor& base, const Tensor& u, const Tensor& P, double scale) {
  Op op("swiglu_bwd_lowrank", gu, "gu");
  const auto [N, F] = swiglu_dims(op, gu);
  op.half_only(gu, "gu");
  op.dims(P, 2, "P");
  const int r = op.to_int(P.size(0), "rank");
  TORCH_CHECK(bllm::swiglu_bwd_lr_ok(r, F), "swiglu_bwd_lowrank: needs rank 16 and F % 8 == 0, got ", r, ", ", F);
  op.shaped(P, {r, F}, gu.scalar_type(), "P");
  op.rows(base, N, F, gu.scalar_type(), "base");
  op.rows(u, N, r, gu.scalar_type(), "u", false, u.element_size());
  auto dgu = at::empty_like(gu);
  bllm::swiglu_bwd_lr(dt_of(gu), gu.data_ptr(), base.data_ptr(), base.stride(0), u.data_ptr(), u.stride(0),
                      P.data_ptr(), r, (float)scale, dgu.data_ptr(), N, F, stream());
  return dgu;
}

// swiglu_bwd_lowrank that also accumulates the LoRA gradients reading the same rows:
// gB_gate (+)= st[:, :16]^T dg, gB_up (+)= st[:, 16:32]^T du (the gate/up group's dB, st = s t), and
// gA_down_t (+)= scale u^T act (the down projection's dA, a [16, F] view of its [F, 16] gradient)
Tensor swiglu_bwd_lowrank_wgrad(const Tensor& gu, const Tensor& base, const Tensor& u, const Tensor& P, double scale,
                                const Tensor& st, Tensor& gB_gate, Tensor& gB_up, Tensor& gA_down_t, bool accumulate) {
  Op op("swiglu_bwd_lowrank_wgrad", gu, "gu");
  const auto [N, F] = swiglu_dims(op, gu);
  op.half_only(gu, "gu");
  op.dims(P, 2, "P");
  const int r = op.to_int(P.size(0), "rank");
  TORCH_CHECK(bllm::swiglu_bwd_lr_wgrad_ok(r, F), "swiglu_bwd_lowrank_wgrad: needs rank 16 and F % 64 == 0, got ", r,
              ", ", F);
  op.shaped(P, {r, F}, gu.scalar_type(), "P");
  op.rows(base, N, F, gu.scalar_type(), "base");
  op.rows(u, N, 16, gu.scalar_type(), "u", /*at_least=*/true);
  op.rows(st, N, 32, gu.scalar_type(), "st", /*at_least=*/true);
  const Tensor* gs[3] = {&gB_gate, &gB_up, &gA_down_t};
  const char* names[3] = {"gB_gate", "gB_up", "gA_down_t"};
  for (int m = 0; m < 3; ++m) {
    op.grad_block(*gs[m], 16, F, names[m]);
    op.dtype(*gs[m], gB_gate.scalar_type(), names[m]);
  }
  const DType odt = dt_of(gB_gate);
  auto dgu = at::empty_like(gu);
  const int S = bllm::swiglu_bwd_lr_wgrad_splits(N, F);
  auto part = at::empty({S, 3 * 16 * (int64_t)F}, gu.options().dtype(at::kFloat));
  bllm::swiglu_bwd_lr_wgrad(dt_of(gu), gu.data_ptr(), base.data_ptr(), base.stride(0), u.data_ptr(), u.stride(0),
                            P.data_ptr(), st.data_ptr(), st.stride(0), (float)scale, dgu.data_ptr(),
                            part.data_ptr<float>(), N, F, S, stream());
  bllm::LoraWgradArgs a{};
  a.accumulate = accumulate;
  a.n = 3;
  for (int m = 0; m < 3; ++m) {
    a.r[m] = 16; a.len[m] = F; a.sa[m] = gs[m]->stride(0); a.sb[m] = gs[m]->stride(1);
    a.gt[m][0] = gs[m]->data_ptr();
    a.part_off[m] = (int64_t)m * 16 * F;
  }
  a.part = part.data_ptr<float>(); a.part_ld = 3 * 16 * (int64_t)F;
  bllm::lora_reduce(odt, a, S, stream());
  return dgu;
}

// ------------------------------------------------------------------ RoPE
// qkv [rows, (H + 2G) hd] contiguous, rotated in place with the fp32 [ctx, hd/2] tables -> {H, G, hd}
std::tuple<int, int, int> rope_args(const Op& op, const Tensor& qkv, const Tensor& cos, const Tensor& sin, int64_t H,
                                    int64_t G, int64_t hd) {
  op.dense(qkv, "qkv");
  TORCH_CHECK(H > 0 && G > 0 && hd > 0 && hd % 2 == 0 && qkv.dim() == 2 && qkv.size(1) == (H + 2 * G) * hd,
              op.name, ": qkv must be [rows, (H + 2G) hd] with an even hd, got ", qkv.sizes(), " for ", H, ", ", G,
              ", ", hd);
  op.to_int(qkv.size(1), "the qkv row length");
  op.shaped(cos, {-1, hd / 2}, at::kFloat, "cos");
  op.like(sin, cos, "sin");
  return {op.to_int(H, "H"), op.to_int(G, "G"), op.to_int(hd, "hd")};
}

void rope_(Tensor& qkv, const Tensor& cos, const Tensor& sin, int64_t T, int64_t H, int64_t G, int64_t hd,
           bool inverse, int64_t pos_offset) {
  Op op("rope_", qkv, "qkv");
  const auto [h, g, d] = rope_args(op, qkv, cos, sin, H, G, hd);
  TORCH_CHECK(T > 0 && pos_offset >= 0 && cos.size(0) >= T + pos_offset, "rope_: T ", T, " at pos_offset ", pos_offset,
              " must be positive / non-negative and fit the tables' ", cos.size(0), " rows");
  bllm::rope(dt_of(qkv), qkv.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), qkv.size(0), op.to_int(T, "T"),
             h, g, d, inverse, op.to_int(pos_offset, "pos_offset"), stream());
}

// graph-replayable RoPE of one decode token: position = pos_offset + *pos (device int32)
void rope_dev_(Tensor& qkv, const Tensor& cos, const Tensor& sin, int64_t H, int64_t G, int64_t hd,
               const Tensor& pos) {
  Op op("rope_dev_", qkv, "qkv");
  const auto [h, g, d] = rope_args(op, qkv, cos, sin, H, G, hd);
  op.vec(pos, 1, at::kInt, "pos");
  // T = 1: every row is one token at position *pos (the caller keeps *pos < cos.size(0))
  bllm::rope(dt_of(qkv), qkv.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), qkv.size(0), 1, h, g, d, false,
             0, stream(), pos.data_ptr<int>());
}

// RoPE of a packed variable-length batch: row r at position pos_ids[r] (int32 [N])
void rope_pos_(Tensor& qkv, const Tensor& cos, const Tensor& sin, const Tensor& pos_ids, int64_t H, int64_t G,
               int64_t hd, bool inverse) {
  Op op("rope_pos_", qkv, "qkv");
  const auto [h, g, d] = rope_args(op, qkv, cos, sin, H, G, hd);
  op.vec(pos_ids, qkv.size(0), at::kInt, "pos_ids");
  bllm::rope_pos(dt_of(qkv), qkv.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), pos_ids.data_ptr<int>(),
                 qkv.size(0), h, g, d, inverse, stream());
}

// ------------------------------------------------------------------ bias gradients and partial sums
// dy [N, F] contiguous with rows of whole 16-B vectors -> {N, F}
std::pair<int, int> colsum_rows(const Op& op, const Tensor& dy, const char* what) {
  op.floating(dy, what);
  op.contig(dy, what);
  TORCH_CHECK(dy.dim() == 2 && dy.size(1) % (16 / dy.element_size()) == 0, op.name, ": ", what,
              " must be [N, F] with F a multiple of 16 bytes, got ", dy.sizes());
  return {op.to_int(dy.size(0), "N"), op.to_int(dy.size(1), "F")};
}

// db (+)= dy.sum(0): dy [N, F] bf16/fp16/fp32, db [F] any float dtype (written in place)
void bias_grad_(const Tensor& dy, Tensor& db, bool accumulate) {
  Op op("bias_grad_", dy, "dy");
  const auto [N, F] = colsum_rows(op, dy, "dy");
  op.floating(db, "db");
  op.shaped(db, {F}, db.scalar_type(), "db");
  auto part = at::empty({bllm::colsum_bands(N, F), F}, dy.options().dtype(at::kFloat));
  bllm::bias_grad(dt_of(dy), dt_of(db), dy.data_ptr(), part.data_ptr<float>(), db.data_ptr(), N, F, accumulate,
                  stream());
}

// fused elementwise backward + bias grad: op 0 = dropout backward of src (p, seed, offset),
// op 1 = exact-GELU backward (src = dg, aux = f); returns the elementwise result, db (+)= its column sums
// db None: no bias sums; act_inplace (op 1): src is overwritten with gelu(aux)
Tensor bwd_bias_grad_(Tensor& src, const optional<Tensor>& aux, const optional<Tensor>& db_, bool accumulate,
                      int64_t kind, double p, int64_t seed, int64_t offset, bool act_inplace) {
  Op op("bwd_bias_grad_", src, "src");
  const auto [N, F] = colsum_rows(op, src, "src");
  const Tensor* db = opt(db_);
  if (db) {
    op.floating(*db, "db");
    op.shaped(*db, {F}, db->scalar_type(), "db");
  }
  TORCH_CHECK(kind == 0 || kind == 1, "bwd_bias_grad_: op must be 0 (dropout) or 1 (GELU), got ", kind);
  TORCH_CHECK(!act_inplace || kind == 1, "bwd_bias_grad_: act_inplace only with the GELU backward");
  if (kind == 1) {
    TORCH_CHECK(aux.has_value(), "bwd_bias_grad_: the GELU backward needs aux");
    op.like(*aux, src, "aux");
  }
  auto out = at::empty_like(src);
  Tensor part;
  if (db) part = at::empty({bllm::colsum_bands(N, F), F}, src.options().dtype(at::kFloat));
  bllm::bwd_bias_grad(dt_of(src), db ? dt_of(*db) : dt_of(src), op.to_int(kind), src.data_ptr(),
                      kind == 1 ? aux->data_ptr() : nullptr, out.data_ptr(), db ? part.data_ptr<float>() : nullptr,
                      opt_ptr(db), N, F, accumulate, (float)p, (uint64_t)seed, (uint64_t)offset,
                      act_inplace ? src.data_ptr() : nullptr, stream());
  return out;
}

// out (+)= part.sum(0): part [S, ...] any float dtype, out contiguous with part[0]'s numel
void sum_partials_(const Tensor& part, Tensor& out, bool accumulate) {
  Op op("sum_partials_", part, "part");
  op.dense(part, "part");
  op.dense(out, "out");
  TORCH_CHECK(part.dim() >= 1, "sum_partials_: part must be [S, ...]");
  const int64_t S = part.size(0), n = out.numel();
  TORCH_CHECK(part.numel() == S * n && n % 8 == 0, "sum_partials_: part ", part.sizes(), " must hold S x ", n,
              " elements (out.numel(), a multiple of 8)");
  bllm::sum_partials_into(dt_of(part), dt_of(out), part.data_ptr(), out.data_ptr(), n, op.to_int(S, "S"), accumulate,
                          stream());
}

// ------------------------------------------------------------------ GEMM (MFMA kernels)
// placement experiments / tests: tile maps of the dW and forward-layout GEMM kernels
void set_gemm_tile_maps(int64_t wg_map, int64_t wg_gm, int64_t nt_map, int64_t nt_gm) {
  bllm::set_wgrad_tile_map((int)wg_map, (int)wg_gm);
  bllm::set_gemm_nt_tile_map((int)nt_map, (int)nt_gm);
}

// Operands of c [M, N] (+)= a^T b (TN: a [K, M], b [K, N]), a b (NN: a [M, K], b [K, N]) or a b^T
// (NT: a [M, K], b [N, K]).  a and b: bf16/fp16 of one dtype, unit column stride, 16-B aligned base
// and row pitch, pitch <= kMaxGemmPitch elements; c: unit column stride,
// base and pitch multiples of c_align bytes, dtype a's (c_dt 2), a's or fp32 (1) or any float dtype (0); dims < 2^31
enum class Gemm { TN, NN, NT };
struct GemmDims { int M, N, K; };
// The LDS-DMA staging of the MFMA GEMMs adds a per-lane uint32_t BYTE offset
// (row * ld + 8 * chunk) * 2 to a 64-bit wave-uniform base (csrc/gemm_wgrad.hip voffA / voffB, voA / voB;
// csrc/gemm_nt.hip voA / voB).  It is exact while (rmax * ld + 8 * cmax) * 2 < 2^32, with
//   wgrad_gemm_k, token-major operands (loaders are waves 0-3): rmax = (3*4+3)*2+1 = 31, cmax = 31
//                                                               -> ld <= 69,273,658
//   wgrad4_k:   rmax = 16*3 + 2*7 + 1 = 63, cmax = 31          -> ld <= 34,087,038
//   wgrad_gemm_k<AK> (gemm_nn's A): rmax = (3*4+3)*16 + 15 = 255, cmax = 3
//                                                               -> ld <= (2^31 - 24 - 1) / 255 = 8,421,504
//   gemm_nt4p_k: *_supported asks 256 * ld * 2 < 2^31 on top of this (its rows reach 63, plus K * 2 bytes;
//               the SwiGLU form's B rows reach F + 127: gemm_nt_swiglu_supported)
// One bound for every operand, the minimum (the widest real pitch is 128,320): above it an offset
// wraps mod 2^32 to a lower address that is still inside the tensor: wrong data, no fault.
constexpr int64_t kMaxGemmPitch = 8421504;
GemmDims gemm_operands(const Op& op, Gemm lay, const Tensor& a, const char* an, const Tensor& b, const char* bn,
                       const Tensor& c, const char* cn, int64_t c_align, int c_dt) {
  op.dims(a, 2, an);
  op.dims(b, 2, bn);
  op.half_only(a, an);
  const int64_t M = a.size(lay == Gemm::TN ? 1 : 0), K = a.size(lay == Gemm::TN ? 0 : 1);
  const int64_t N = b.size(lay == Gemm::NT ? 0 : 1);
  op.rows(a, -1, -1, a.scalar_type(), an);
  op.rows(b, lay == Gemm::NT ? N : K, lay == Gemm::NT ? K : N, a.scalar_type(), bn);
  TORCH_CHECK(a.stride(0) <= kMaxGemmPitch && b.stride(0) <= kMaxGemmPitch, op.name, ": row stride of ", an, " / ",
              bn, " too large: ", a.stride(0), ", ", b.stride(0), " (at most ", kMaxGemmPitch, " elements)");
  op.floating(c, cn);
  const bool own = c_dt == 0 || (c_dt == 1 && c.scalar_type() == at::kFloat);
  op.rows(c, M, N, own ? c.scalar_type() : a.scalar_type(), cn, false, c_align ? c_align : c.element_size());
  return {op.to_int(M, "M"), op.to_int(N, "N"), op.to_int(K, "K")};
}

// c (+)= a^T b on the token-major MFMA kernel: a [K, M], b [K, N], c [M, N], unit column
// strides, 16-B aligned rows; splits > 1 reduce K ranges into fp32 partials summed in order
void wgrad_gemm_(const Tensor& a, const Tensor& b, Tensor& c, bool accumulate, int64_t splits) {
  Op op("wgrad_gemm_", a, "a");
  const auto [M, N, K] = gemm_operands(op, Gemm::TN, a, "a", b, "b", c, "c", 0, 0);
  const int S = op.to_int(splits, "splits");
  TORCH_CHECK(bllm::wgrad_gemm_supported(M, N, K, S), "wgrad_gemm_: unsupported shape ", K, "x", M, "x", N, " splits ",
              splits);
  if (S == 1) {
    bllm::wgrad_gemm(dt_of(a), dt_of(c), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(),
                     c.stride(0), 0, M, N, K, 1, accumulate, stream());
    return;
  }
  TORCH_CHECK(c.is_contiguous(), "wgrad_gemm_: the split-K output c must be contiguous");
  auto part = at::empty({S, M, N}, a.options().dtype(at::kFloat));
  bllm::wgrad_gemm(dt_of(a), DType::F32, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), part.data_ptr(), N,
                   (int64_t)M * N, M, N, K, S, false, stream());
  bllm::sum_partials_into(DType::F32, dt_of(c), part.data_ptr(), c.data_ptr(), (int64_t)M * N, S, accumulate,
                          stream());
}

// c (+)= a^T b with the grouped tile order in two launches: tiles [0, full) whole-K straight into c,
// the remaining tiles split St ways over K into compact fp32 partials summed into c afterwards
void wgrad_gemm_tail_(const Tensor& a, const Tensor& b, Tensor& c, bool accumulate, int64_t full, int64_t St) {
  Op op("wgrad_gemm_tail_", a, "a");
  const auto [M, N, K] = gemm_operands(op, Gemm::TN, a, "a", b, "b", c, "c", 16, 0);
  TORCH_CHECK(c.stride(0) % 8 == 0, "wgrad_gemm_tail_: the row stride of c must be a multiple of 8 elements");
  const int nfull = op.to_int(full, "full"), S = op.to_int(St, "St");
  TORCH_CHECK(bllm::wgrad_tail_supported(M, N, K, nfull, S), "wgrad_gemm_tail_: unsupported ", K, "x", M, "x", N,
              " full ", full, " splits ", St);
  const int64_t tail = (M / 256) * (N / 256) - nfull;
  auto part = at::empty({S * tail * 256 * 256}, a.options().dtype(at::kFloat));
  bllm::wgrad_gemm_tail(dt_of(a), dt_of(c), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(),
                        c.stride(0), M, N, K, nfull, S, part.data_ptr<float>(), accumulate, stream());
}

// c [M, N] (+)= a [M, K] . b [K, N], all row-major (input gradient dX = dY W of a Linear)
void gemm_nn_(const Tensor& a, const Tensor& b, Tensor& c, bool accumulate) {
  Op op("gemm_nn_", a, "a");
  const auto [M, N, K] = gemm_operands(op, Gemm::NN, a, "a", b, "b", c, "c", 0, 1);
  TORCH_CHECK(bllm::gemm_nn_supported(M, N, K), "gemm_nn_: unsupported shape ", M, "x", N, "x", K);
  bllm::gemm_nn(dt_of(a), dt_of(c), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0),
                M, N, K, accumulate, stream());
}

// c[M, N] (+)= a[M, K] . b[N, K]^T on the MFMA kernel (both operands K-contiguous)
void gemm_nt_(const Tensor& a, const Tensor& b, Tensor& c, bool accumulate) {
  Op op("gemm_nt_", a, "a");
  const auto [M, N, K] = gemm_operands(op, Gemm::NT, a, "a", b, "b", c, "c", 0, 1);
  TORCH_CHECK(bllm::gemm_nt2_supported(M, N, K, a.stride(0), b.stride(0)), "gemm_nt_: unsupported shape ", M, "x", N,
              "x", K);
  bllm::gemm_nt2(dt_of(a), dt_of(c), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(),
                 c.stride(0), M, N, K, accumulate, stream());
}

// gate/up projection + SwiGLU forward in one kernel (csrc/gemm_nt.hip): gu[M, 2F] = a . w^T with
// w = [W_gate; W_up] ([2F, K]) and act[M, F] = silu(gu[:, :F]) * gu[:, F:]
void gemm_nt_swiglu_(const Tensor& a, const Tensor& w, Tensor& gu, Tensor& act) {
  Op op("gemm_nt_swiglu_", a, "a");
  const auto [M, N, K] = gemm_operands(op, Gemm::NT, a, "a", w, "w", gu, "gu", 16, 2);
  const int F = N / 2;
  TORCH_CHECK(N == 2 * F, "gemm_nt_swiglu_: w must be [2F, K], got ", w.sizes());
  op.shaped(act, {M, F}, a.scalar_type(), "act");
  TORCH_CHECK(aligned(act, 16), "gemm_nt_swiglu_: act must be 16-B aligned");
  TORCH_CHECK(bllm::gemm_nt_swiglu_supported(M, F, K, a.stride(0), w.stride(0), gu.stride(0)),
              "gemm_nt_swiglu_: unsupported shape ", M, "x", F, "x", K);
  bllm::gemm_nt_swiglu(dt_of(a), a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), gu.data_ptr(), gu.stride(0),
                       act.data_ptr(), M, F, K, stream());
}

// QKV projection with RoPE in the epilogue (K4, csrc/gemm_nt.hip): qkv[M, N] = a . w^T, columns
// below nrot rotated at position row % T (tables fp32 [>= T, 64], head dim 128)
void gemm_nt_rope_(const Tensor& a, const Tensor& w, Tensor& qkv, const Tensor& cos, const Tensor& sin, int64_t T,
                   int64_t nrot, int64_t hd) {
  Op op("gemm_nt_rope_", a, "a");
  const auto [M, N, K] = gemm_operands(op, Gemm::NT, a, "a", w, "w", qkv, "qkv", 8, 2);
  TORCH_CHECK(bllm::gemm_nt_rope_supported(M, N, K, a.stride(0), w.stride(0), qkv.stride(0), op.to_int(hd, "hd")),
              "gemm_nt_rope_: unsupported shape ", M, "x", N, "x", K, " hd ", hd);
  op.shaped(cos, {-1, hd / 2}, at::kFloat, "cos");
  op.like(sin, cos, "sin");
  TORCH_CHECK(T > 0 && cos.size(0) >= T, "gemm_nt_rope_: the tables have ", cos.size(0), " rows, T = ", T);
  TORCH_CHECK(nrot >= 0 && nrot % hd == 0 && nrot <= N, "gemm_nt_rope_: nrot must be whole heads within N, got ", nrot);
  bllm::gemm_nt_rope(dt_of(a), a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), qkv.data_ptr(), qkv.stride(0),
                     M, N, K, cos.data_ptr<float>(), sin.data_ptr<float>(), op.to_int(T, "T"), op.to_int(nrot),
                     stream());
}

// GPT-2 c_fc with bias + exact GELU in the epilogue (K9, csrc/gemm_nt.hip): f = a . w^T + bias,
// g = gelu(f); f and g contiguous [M, N]
void gemm_nt_bias_gelu_(const Tensor& a, const Tensor& w, const Tensor& bias, Tensor& f, Tensor& g) {
  Op op("gemm_nt_bias_gelu_", a, "a");
  const auto [M, N, K] = gemm_operands(op, Gemm::NT, a, "a", w, "w", f, "f", 8, 2);
  op.contig(f, "f");
  op.like(g, f, "g");
  op.vec(bias, N, a.scalar_type(), "bias");
  TORCH_CHECK(aligned(g, 8) && aligned(bias, 8), "gemm_nt_bias_gelu_: g and bias must be 8-B aligned");
  TORCH_CHECK(bllm::gemm_nt_bias_gelu_supported(M, N, K, a.stride(0), w.stride(0), f.stride(0)),
              "gemm_nt_bias_gelu_: unsupported shape ", M, "x", N, "x", K);
  bllm::gemm_nt_bias_gelu(dt_of(a), a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), bias.data_ptr(),
                          f.data_ptr(), g.data_ptr(), f.stride(0), M, N, K, stream());
}

// ------------------------------------------------------------------ attention
// kc / vc [B, G, Tmax, hd]: contiguous caches of q's dtype, head dim 64 or 128, H a multiple of G
void decode_caches(const Op& op, const Tensor& q, const Tensor& kc, const Tensor& vc, int64_t B, int64_t H,
                   int64_t hd) {
  op.half_only(q, "q / qkv");
  op.contig(q, "q / qkv");
  op.shaped(kc, {B, -1, -1, hd}, q.scalar_type(), "kcache");
  op.like(vc, kc, "vcache");
  TORCH_CHECK(hd == 64 || hd == 128, op.name, ": head_dim 64 or 128, got ", hd);
  TORCH_CHECK(B > 0 && H > 0 && kc.size(1) > 0 && H % kc.size(1) == 0, op.name, ": B ", B, " and H ", H,
              " must be positive and H a multiple of the cache's G ", kc.size(1));
}

// qkv [B, (H+2G)*hd] (one decode token per row); kc / vc [B, G, Tmax, hd] valid below *pos;
// appends the token's k / v at *pos and attends over pos + 1 keys -> out [B, H*hd]
Tensor attn_decode_append(const Tensor& qkv, Tensor& kc, Tensor& vc, const Tensor& pos, int64_t H, int64_t G) {
  Op op("attn_decode_append", qkv, "qkv");
  op.dims(qkv, 2, "qkv");
  op.dims(kc, 4, "kcache");
  const int64_t B = qkv.size(0), hd = kc.size(3), Tmax = kc.size(2);
  decode_caches(op, qkv, kc, vc, B, H, hd);
  TORCH_CHECK(kc.size(1) == G && qkv.size(1) == (H + 2 * G) * hd, "attn_decode_append: qkv ", qkv.sizes(),
              " / cache ", kc.sizes(), " mismatch for H ", H, " G ", G);
  TORCH_CHECK(Tmax <= bllm::attn_decode_max_len(), "attn_decode_append: cache longer than the LDS score buffer");
  op.vec(pos, 1, at::kInt, "pos");
  auto out = at::empty({B, H * hd}, qkv.options());
  bllm::attn_decode_append(dt_of(qkv), qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                           pos.data_ptr<int>(), op.to_int(B, "B"), op.to_int(H, "H"), op.to_int(G, "G"),
                           op.to_int(hd, "hd"), op.to_int(Tmax, "Tmax"), stream());
  return out;
}

// attn_decode_append with a position per batch row: pos int32 [B], row b appends at pos[b] and
// attends over pos[b] + 1 keys (the caller keeps every pos[b] < Tmax)
Tensor attn_decode_append_rows(const Tensor& qkv, Tensor& kc, Tensor& vc, const Tensor& pos, int64_t H, int64_t G) {
  Op op("attn_decode_append_rows", qkv, "qkv");
  op.dims(qkv, 2, "qkv");
  op.dims(kc, 4, "kcache");
  const int64_t B = qkv.size(0), hd = kc.size(3), Tmax = kc.size(2);
  decode_caches(op, qkv, kc, vc, B, H, hd);
  TORCH_CHECK(kc.size(1) == G && qkv.size(1) == (H + 2 * G) * hd, "attn_decode_append_rows: qkv ", qkv.sizes(),
              " / cache ", kc.sizes(), " mismatch for H ", H, " G ", G);
  TORCH_CHECK(Tmax >= 1 && Tmax <= bllm::attn_decode_max_len(),
              "attn_decode_append_rows: cache empty or longer than the LDS score buffer");
  op.vec(pos, B, at::kInt, "pos");
  auto out = at::empty({B, H * hd}, qkv.options());
  bllm::attn_decode_append_rows(dt_of(qkv), qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                                pos.data_ptr<int>(), op.to_int(B, "B"), op.to_int(H, "H"), op.to_int(G, "G"),
                                op.to_int(hd, "hd"), op.to_int(Tmax, "Tmax"), stream());
  return out;
}

// qkv [N, (H+2G)*hd] packed rows, sequence b = rows [cu[b], cu[b+1]) (cu int32 [B+1], lengths
// <= Tmax: the caller's host bounds); kc / vc [B, G, Tmax, hd]: rows t < len_b of (b, g) <- the k / v
// of qkv row cu[b] + t, nothing else written.  rows (int32 [n], n <= B): the batch has n sequences
// (cu int32 [n+1]) and sequence i goes to cache row rows[i]; the host wrapper has checked the values
// distinct and inside [0, B), the kernel skips a row outside that range
int fill_rows(const Op& op, const optional<Tensor>& rows_, const Tensor& cu, int64_t B, const int** rows) {
  *rows = nullptr;
  if (const Tensor* r = opt(rows_)) {
    op.contig(*r, "rows");
    op.dtype(*r, at::kInt, "rows");
    TORCH_CHECK(r->dim() == 1 && r->numel() <= B, op.name, ": rows must be 1-D with at most the cache's ", B,
                " rows, got ", r->sizes());
    op.vec(cu, r->numel() + 1, at::kInt, "cu");
    *rows = r->data_ptr<int>();
    return op.to_int(r->numel(), "sequences");
  }
  op.vec(cu, B + 1, at::kInt, "cu");
  return op.to_int(B, "B");
}

void kv_cache_fill_varlen(const Tensor& qkv, const Tensor& cu, Tensor& kc, Tensor& vc,
                          const optional<Tensor>& rows_) {
  Op op("kv_cache_fill_varlen", qkv, "qkv");
  op.dense(qkv, "qkv");
  op.dims(qkv, 2, "qkv");
  op.dims(kc, 4, "kcache");
  const int64_t N = qkv.size(0), B = kc.size(0), G = kc.size(1), Tmax = kc.size(2), hd = kc.size(3);
  op.shaped(kc, {B, G, Tmax, hd}, qkv.scalar_type(), "kcache");
  op.like(vc, kc, "vcache");
  const int64_t row_bytes = hd * qkv.element_size();
  TORCH_CHECK(B > 0 && G > 0 && Tmax > 0 && hd > 0 && row_bytes % 16 == 0 && aligned(qkv, 16) && aligned(kc, 16) &&
                  aligned(vc, 16),
              "kv_cache_fill_varlen: cache ", kc.sizes(), " must be non-empty with 16-byte aligned head rows");
  TORCH_CHECK(qkv.size(1) % hd == 0 && qkv.size(1) / hd > 2 * G, "kv_cache_fill_varlen: qkv ", qkv.sizes(),
              " is not [N, (H + 2G) hd] for the cache's G ", G, " and hd ", hd);
  const int* rows;
  const int nseq = fill_rows(op, rows_, cu, B, &rows);
  bllm::kv_cache_fill_varlen(qkv.data_ptr(), cu.data_ptr<int>(), kc.data_ptr(), vc.data_ptr(), N, nseq,
                             op.to_int(qkv.size(1) / hd - 2 * G, "H"), op.to_int(G, "G"), op.to_int(Tmax, "Tmax"),
                             op.to_int(row_bytes, "row bytes"), stream(), rows, op.to_int(B, "B"));
}

// q [B, H, hd]; kc / vc [B, G, Tmax, hd] with the first L positions valid -> out [B, H*hd]
Tensor attn_decode(const Tensor& q, const Tensor& kc, const Tensor& vc, int64_t L) {
  Op op("attn_decode", q, "q");
  op.dims(q, 3, "q");
  op.dims(kc, 4, "kcache");
  const int64_t B = q.size(0), H = q.size(1), hd = q.size(2), G = kc.size(1), Tmax = kc.size(2);
  decode_caches(op, q, kc, vc, B, H, hd);
  TORCH_CHECK(L >= 1 && L <= Tmax && L <= bllm::attn_decode_max_len(), "attn_decode: bad length ", L);
  auto out = at::empty({B, H * hd}, q.options());
  bllm::attn_decode(dt_of(q), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), op.to_int(B, "B"),
                    op.to_int(H, "H"), op.to_int(G, "G"), op.to_int(hd, "hd"), op.to_int(Tmax, "Tmax"),
                    op.to_int(L, "L"), stream());
  return out;
}

// Split-KV forms of the two ops above (csrc/attn_decode_split.hip): any cache length, the key
// chunks fixed by Tmax.  The scratch of per-chunk partials is allocated here per call (under graph
// capture it belongs to the graph's pool); the merge reads only the slots this call wrote.
Tensor decode_split_scratch(const Op& op, const Tensor& q, int64_t B, int64_t H, int64_t G, int64_t hd,
                            int64_t Tmax) {
  TORCH_CHECK(Tmax >= 1, op.name, ": empty cache");
  op.to_int(Tmax, "Tmax");
  TORCH_CHECK(bllm::attn_decode_split_grid_ok(op.to_int(B, "B"), op.to_int(H, "H"), op.to_int(G, "G")), op.name,
              ": B ", B, " or the cache's G ", G, " exceeds the launch grid");
  return at::empty({bllm::attn_decode_split_workspace((int)B, (int)H, (int)hd, (int)Tmax)},
                   q.options().dtype(at::kFloat));
}

// attn_decode_append / attn_decode_append_rows in one: pos int32 with 1 element (a position
// shared by the rows) or B elements (one per row; the caller keeps every position < Tmax)
Tensor attn_decode_append_split(const Tensor& qkv, Tensor& kc, Tensor& vc, const Tensor& pos, int64_t H, int64_t G) {
  Op op("attn_decode_append_split", qkv, "qkv");
  op.dims(qkv, 2, "qkv");
  op.dims(kc, 4, "kcache");
  const int64_t B = qkv.size(0), hd = kc.size(3), Tmax = kc.size(2);
  decode_caches(op, qkv, kc, vc, B, H, hd);
  TORCH_CHECK(kc.size(1) == G && qkv.size(1) == (H + 2 * G) * hd, "attn_decode_append_split: qkv ", qkv.sizes(),
              " / cache ", kc.sizes(), " mismatch for H ", H, " G ", G);
  TORCH_CHECK(aligned(qkv, 16) && aligned(kc, 16) && aligned(vc, 16),
              "attn_decode_append_split: qkv and the caches must be 16-byte aligned");
  op.contig(pos, "pos");
  op.dtype(pos, at::kInt, "pos");
  TORCH_CHECK(pos.numel() == 1 || pos.numel() == B, "attn_decode_append_split: pos must have 1 or ", B,
              " elements, got ", pos.numel());
  auto ws = decode_split_scratch(op, qkv, B, H, G, hd, Tmax);
  auto out = at::empty({B, H * hd}, qkv.options());
  bllm::attn_decode_append_split(dt_of(qkv), qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                                 ws.data_ptr<float>(), pos.data_ptr<int>(), pos.numel() == 1 ? 0 : 1, (int)B, (int)H,
                                 (int)G, (int)hd, (int)Tmax, stream());
  return out;
}

// q [B, H, hd]; kc / vc [B, G, Tmax, hd] with the first L positions valid -> out [B, H*hd]
Tensor attn_decode_split(const Tensor& q, const Tensor& kc, const Tensor& vc, int64_t L) {
  Op op("attn_decode_split", q, "q");
  op.dims(q, 3, "q");
  op.dims(kc, 4, "kcache");
  const int64_t B = q.size(0), H = q.size(1), hd = q.size(2), G = kc.size(1), Tmax = kc.size(2);
  decode_caches(op, q, kc, vc, B, H, hd);
  TORCH_CHECK(aligned(q, 16) && aligned(kc, 16) && aligned(vc, 16),
              "attn_decode_split: q and the caches must be 16-byte aligned");
  TORCH_CHECK(L >= 1 && L <= Tmax, "attn_decode_split: bad length ", L);
  auto ws = decode_split_scratch(op, q, B, H, G, hd, Tmax);
  auto out = at::empty({B, H * hd}, q.options());
  bllm::attn_decode_split(dt_of(q), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), ws.data_ptr<float>(),
                          (int)B, (int)H, (int)G, (int)hd, (int)Tmax, (int)L, stream());
  return out;
}
int64_t attn_decode_split_chunk() { return bllm::attn_decode_split_chunk(); }

// FP8 KV cache (csrc/attn_decode_fp8.hip): k8 / v8 [B, G, Tmax, hd] e4m3fn, ks / vs [B, G, Tmax] fp32,
// all contiguous and 16-byte aligned; qkv bf16 / fp16, hd 64 or 128 -> (B, G, Tmax, hd) of the cache
std::tuple<int64_t, int64_t, int64_t, int64_t> fp8_caches(const Op& op, const Tensor& qkv, const Tensor& k8,
                                                          const Tensor& ks, const Tensor& v8, const Tensor& vs) {
  op.half_only(qkv, "qkv");
  op.contig(qkv, "qkv");
  op.dims(qkv, 2, "qkv");
  op.dims(k8, 4, "kcache");
  const int64_t B = k8.size(0), G = k8.size(1), Tmax = k8.size(2), hd = k8.size(3);
  op.shaped(k8, {B, G, Tmax, hd}, at::kFloat8_e4m3fn, "kcache");
  op.like(v8, k8, "vcache");
  op.shaped(ks, {B, G, Tmax}, at::kFloat, "kscale");
  op.like(vs, ks, "vscale");
  TORCH_CHECK(hd == 64 || hd == 128, op.name, ": head_dim 64 or 128, got ", hd);
  TORCH_CHECK(B > 0 && G > 0 && Tmax > 0, op.name, ": empty cache ", k8.sizes());
  op.to_int(Tmax, "Tmax");
  TORCH_CHECK(aligned(qkv, 16) && aligned(k8, 16) && aligned(v8, 16) && aligned(ks, 4) && aligned(vs, 4), op.name,
              ": qkv and the caches must be 16-byte aligned");
  return {B, G, Tmax, hd};
}

// kv_cache_fill_varlen into an fp8 cache: rows t < len_b of (b, g) <- the quantised k / v of qkv
// row cu[b] + t and their scales, nothing else written; rows as in kv_cache_fill_varlen
void kv_cache_fill_varlen_fp8(const Tensor& qkv, const Tensor& cu, Tensor& k8, Tensor& ks, Tensor& v8, Tensor& vs,
                              const optional<Tensor>& rows_) {
  Op op("kv_cache_fill_varlen_fp8", qkv, "qkv");
  const auto [B, G, Tmax, hd] = fp8_caches(op, qkv, k8, ks, v8, vs);
  TORCH_CHECK(qkv.size(1) % hd == 0 && qkv.size(1) / hd > 2 * G, "kv_cache_fill_varlen_fp8: qkv ", qkv.sizes(),
              " is not [N, (H + 2G) hd] for the cache's G ", G, " and hd ", hd);
  const int* rows;
  const int nseq = fill_rows(op, rows_, cu, B, &rows);
  bllm::kv_cache_fill_varlen_fp8(dt_of(qkv), qkv.data_ptr(), cu.data_ptr<int>(), k8.data_ptr(), ks.data_ptr<float>(),
                                 v8.data_ptr(), vs.data_ptr<float>(), qkv.size(0), nseq,
                                 op.to_int(qkv.size(1) / hd - 2 * G, "H"), op.to_int(G, "G"), (int)hd, (int)Tmax,
                                 stream(), rows, op.to_int(B, "B"));
}

// attn_decode_append_rows on an fp8 cache: row b's new k / v are quantised into cache row pos[b]
// (pos int32 [B], the caller keeps every position < Tmax) and its query attends over the
// dequantised keys 0..pos[b] -> out [B, H*hd]
Tensor attn_decode_append_rows_fp8(const Tensor& qkv, Tensor& k8, Tensor& ks, Tensor& v8, Tensor& vs,
                                   const Tensor& pos, int64_t H, int64_t G) {
  Op op("attn_decode_append_rows_fp8", qkv, "qkv");
  const auto [B, Gc, Tmax, hd] = fp8_caches(op, qkv, k8, ks, v8, vs);
  TORCH_CHECK(H > 0 && G > 0 && H % G == 0 && Gc == G && qkv.size(0) == B && qkv.size(1) == (H + 2 * G) * hd,
              "attn_decode_append_rows_fp8: qkv ", qkv.sizes(), " / cache ", k8.sizes(), " mismatch for H ", H, " G ",
              G);
  op.vec(pos, B, at::kInt, "pos");
  auto ws = decode_split_scratch(op, qkv, B, H, G, hd, Tmax);
  auto out = at::empty({B, H * hd}, qkv.options());
  bllm::attn_decode_append_rows_fp8(dt_of(qkv), qkv.data_ptr(), k8.data_ptr(), ks.data_ptr<float>(), v8.data_ptr(),
                                    vs.data_ptr<float>(), out.data_ptr(), ws.data_ptr<float>(), pos.data_ptr<int>(),
                                    (int)B, (int)H, (int)G, (int)hd, (int)Tmax, stream());
  return out;
}

// Q tokens per row over the cache (csrc/attn_extend.hip): qkv [B Q, (H+2G) hd], row b Q + j = token j
// of row b at position pos[b] + j (pos int32 [B], the caller keeps every pos[b] + Q <= Tmax);
// pos_rows int32 [B Q] = pos[b] + j (what the merge launch reads) -> out [B Q, H hd]
Tensor attn_extend_rows(const Tensor& qkv, Tensor& kc, Tensor& vc, const Tensor& pos, const Tensor& pos_rows,
                        int64_t Q, int64_t H, int64_t G) {
  Op op("attn_extend_rows", qkv, "qkv");
  op.dims(qkv, 2, "qkv");
  op.dims(kc, 4, "kcache");
  const int64_t B = kc.size(0), hd = kc.size(3), Tmax = kc.size(2);
  decode_caches(op, qkv, kc, vc, B, H, hd);
  TORCH_CHECK(G > 0 && bllm::attn_extend_supported(op.to_int(Q, "Q"), op.to_int(H, "H"), op.to_int(G, "G")),
              "attn_extend_rows: Q must be in 2..8 with Q * (H / G) <= 32, got Q ", Q, " H ", H, " G ", G);
  TORCH_CHECK(kc.size(1) == G && qkv.size(0) == B * Q && qkv.size(1) == (H + 2 * G) * hd, "attn_extend_rows: qkv ",
              qkv.sizes(), " / cache ", kc.sizes(), " mismatch for Q ", Q, " H ", H, " G ", G);
  TORCH_CHECK(Tmax >= Q, "attn_extend_rows: the cache holds ", Tmax, " positions, fewer than Q = ", Q);
  TORCH_CHECK(aligned(qkv, 16) && aligned(kc, 16) && aligned(vc, 16),
              "attn_extend_rows: qkv and the caches must be 16-byte aligned");
  op.vec(pos, B, at::kInt, "pos");
  op.vec(pos_rows, B * Q, at::kInt, "pos_rows");
  op.to_int(Tmax, "Tmax");
  op.to_int(B * Q * H, "B * Q * H");
  TORCH_CHECK(bllm::attn_extend_grid_ok(op.to_int(B, "B"), (int)G), "attn_extend_rows: B ", B, " or the cache's G ", G,
              " exceeds the launch grid");
  auto ws = at::empty({bllm::attn_extend_workspace((int)B, (int)Q, (int)H, (int)hd, (int)Tmax)},
                      qkv.options().dtype(at::kFloat));
  auto out = at::empty({B * Q, H * hd}, qkv.options());
  bllm::attn_extend_rows(dt_of(qkv), qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                         ws.data_ptr<float>(), pos.data_ptr<int>(), pos_rows.data_ptr<int>(), (int)B, (int)Q, (int)H,
                         (int)G, (int)hd, (int)Tmax, stream());
  return out;
}

// qkv [B T, (H + 2G) hd] contiguous; B, T, H, G, hd positive, H a multiple of G -> them as ints
struct AttnDims { int B, T, H, G, hd; };
AttnDims attn_args(const Op& op, const Tensor& qkv, int64_t B, int64_t T, int64_t H, int64_t G, int64_t hd) {
  op.dense(qkv, "qkv");
  TORCH_CHECK(B > 0 && T > 0 && H > 0 && G > 0 && hd > 0 && H % G == 0, op.name,
              ": B, T, H, G, hd must be positive and H a multiple of G, got ", B, ", ", T, ", ", H, ", ", G, ", ", hd);
  const int d = op.to_int(hd, "hd");
  TORCH_CHECK(bllm::attn_supported_head_dim(d), op.name, ": unsupported head_dim ", hd);
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) == B * T && qkv.size(1) == (H + 2 * G) * hd, op.name,
              ": qkv must be [B T, (H + 2G) hd], got ", qkv.sizes());
  op.to_int(B * T, "B * T");
  return {op.to_int(B, "B"), op.to_int(T, "T"), op.to_int(H, "H"), op.to_int(G, "G"), d};
}

// keep_mask: optional uint32 [B*H, ceil(T/32), T] the forward fills with the dropout keep bits
// (dropout > 0, bf16/fp16) and the backward reads (api.h attn_fwd)
uint32_t* keep_mask_ptr(const Op& op, const optional<Tensor>& m, const Tensor& qkv, const AttnDims& n, double p) {
  if (!m.has_value() || p <= 0.0 || !bllm::attn_keep_mask_ok(dt_of(qkv), n.hd)) return nullptr;
  op.vec(*m, (int64_t)n.B * n.H * ((n.T + 31) / 32) * n.T, at::kInt, "keep_mask (int32 [B*H, ceil(T/32), T])");
  return reinterpret_cast<uint32_t*>(m->data_ptr<int32_t>());
}

// fp32 [>= T, hd/2] RoPE table for the inverse rotation fused into the attention backward
const float* rope_ptr(const Op& op, const optional<Tensor>& o, int64_t T, int64_t hd, const char* what) {
  const Tensor* t = opt(o);
  if (!t) return nullptr;
  op.shaped(*t, {-1, hd / 2}, at::kFloat, what);
  TORCH_CHECK(t->size(0) >= T, op.name, ": ", what, " has ", t->size(0), " rows, needs ", T);
  return t->data_ptr<float>();
}

std::tuple<Tensor, Tensor> flash_attn_fwd(const Tensor& qkv, int64_t B, int64_t T, int64_t H, int64_t G,
                                          int64_t hd, bool causal, double p, int64_t seed, int64_t offset,
                                          const optional<Tensor>& keep_mask) {
  Op op("flash_attn_fwd", qkv, "qkv");
  const AttnDims n = attn_args(op, qkv, B, T, H, G, hd);
  auto o = at::empty({B * T, H * hd}, qkv.options());
  auto lse = at::empty({B, H, T}, qkv.options().dtype(at::kFloat));
  bllm::attn_fwd(dt_of(qkv), qkv.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), n.B, n.T, n.H, n.G, n.hd, causal,
                 (float)p, (uint64_t)seed, (uint64_t)offset, keep_mask_ptr(op, keep_mask, qkv, n, p), stream());
  return {o, lse};
}

Tensor flash_attn_bwd(const Tensor& qkv, const Tensor& o, const Tensor& lse, const Tensor& dout, int64_t B,
                      int64_t T, int64_t H, int64_t G, int64_t hd, bool causal, double p, int64_t seed,
                      int64_t offset, const optional<Tensor>& keep_mask, const optional<Tensor>& rope_cos,
                      const optional<Tensor>& rope_sin) {
  Op op("flash_attn_bwd", qkv, "qkv");
  const AttnDims n = attn_args(op, qkv, B, T, H, G, hd);
  op.shaped(o, {B * T, H * hd}, qkv.scalar_type(), "o");
  op.like(dout, o, "dout");
  op.vec(lse, B * H * T, at::kFloat, "lse");
  const float* rcos = rope_ptr(op, rope_cos, T, hd, "rope_cos");
  const float* rsin = rope_ptr(op, rope_sin, T, hd, "rope_sin");
  TORCH_CHECK(!rcos == !rsin, "flash_attn_bwd: give both rope tables or neither");
  auto dqkv = at::empty_like(qkv);
  auto delta = at::empty({B, H, T}, qkv.options().dtype(at::kFloat));
  // per-query-head dK/dV partials only for GQA (MHA writes dK/dV directly); dQ is atomic-free
  Tensor dkv_part;
  const bool mfma = qkv.scalar_type() != at::kFloat && bllm::attn_mfma_head_dim(n.hd);
  if (mfma && bllm::attn_bwd_kv_partials(n.B, n.T, n.H, n.G))
    dkv_part = at::empty({2, B * T, H, hd}, qkv.options().dtype(at::kFloat));
  bllm::attn_bwd(dt_of(qkv), qkv.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), dout.data_ptr(), dqkv.data_ptr(),
                 delta.data_ptr<float>(), opt_ptr<float>(&dkv_part), n.B, n.T, n.H, n.G, n.hd, causal, (float)p,
                 (uint64_t)seed, (uint64_t)offset, keep_mask_ptr(op, keep_mask, qkv, n, p), rcos, rsin, stream());
  return dqkv;
}

// Variable-length attention (causal, no dropout) on a packed batch: sequence b is rows
// [cu[b], cu[b+1]) of qkv [N, (H+2G) hd]; bf16 / fp16, head dims 64 / 128 (the matrix-core kernels)
// -> {B, max_len, H, G, hd} as ints
AttnDims varlen_args(const Op& op, const Tensor& qkv, const Tensor& cu, int64_t max_len, int64_t H, int64_t G,
                     int64_t hd) {
  op.half_only(qkv, "qkv");
  op.contig(qkv, "qkv");
  TORCH_CHECK(hd == 64 || hd == 128, op.name, ": head_dim 64 or 128, got ", hd);
  TORCH_CHECK(H > 0 && G > 0 && H % G == 0, op.name, ": n_heads must be a positive multiple of n_kv_groups");
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(1) == (H + 2 * G) * hd, op.name, ": qkv must be [N, (H + 2G) hd], got ",
              qkv.sizes());
  op.shaped(cu, {-1}, at::kInt, "cu");
  TORCH_CHECK(cu.numel() >= 1, op.name, ": cu must be int32 [B + 1]");
  TORCH_CHECK(max_len >= 0 && max_len <= qkv.size(0), op.name, ": max_len ", max_len, " outside [0, N]");
  op.to_int(qkv.size(0), "N");
  return {op.to_int(cu.numel() - 1, "B"), op.to_int(max_len, "max_len"), op.to_int(H, "H"), op.to_int(G, "G"),
          op.to_int(hd, "hd")};
}

std::tuple<Tensor, Tensor> flash_attn_varlen_fwd(const Tensor& qkv, const Tensor& cu, int64_t max_len, int64_t H,
                                                 int64_t G, int64_t hd) {
  Op op("flash_attn_varlen_fwd", qkv, "qkv");
  const AttnDims n = varlen_args(op, qkv, cu, max_len, H, G, hd);
  const int64_t N = qkv.size(0);
  auto o = at::empty({N, H * hd}, qkv.options());
  auto lse = at::empty({H * N}, qkv.options().dtype(at::kFloat));
  bllm::attn_fwd_mfma_varlen(dt_of(qkv), qkv.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), cu.data_ptr<int>(),
                             n.B, n.T, n.H, n.G, n.hd, stream());
  return {o, lse};
}

Tensor flash_attn_varlen_bwd(const Tensor& qkv, const Tensor& o, const Tensor& lse, const Tensor& dout,
                             const Tensor& cu, const Tensor& pos_ids, int64_t max_len, int64_t H, int64_t G,
                             int64_t hd, const optional<Tensor>& rope_cos, const optional<Tensor>& rope_sin) {
  Op op("flash_attn_varlen_bwd", qkv, "qkv");
  const AttnDims n = varlen_args(op, qkv, cu, max_len, H, G, hd);
  const int64_t N = qkv.size(0);
  op.shaped(o, {N, H * hd}, qkv.scalar_type(), "o");
  op.like(dout, o, "dout");
  op.vec(lse, H * N, at::kFloat, "lse");
  op.vec(pos_ids, N, at::kInt, "pos_ids");
  const float* rcos = rope_ptr(op, rope_cos, max_len, hd, "rope_cos");
  const float* rsin = rope_ptr(op, rope_sin, max_len, hd, "rope_sin");
  TORCH_CHECK(!rcos == !rsin, "flash_attn_varlen_bwd: give both rope tables or neither");
  auto dqkv = at::empty_like(qkv);
  auto delta = at::empty({H * N}, qkv.options().dtype(at::kFloat));
  Tensor dkv_part;
  if (bllm::attn_bwd_kv_partials(n.B, n.T, n.H, n.G))
    dkv_part = at::empty({2, N, H, hd}, qkv.options().dtype(at::kFloat));
  bllm::attn_bwd_mfma_varlen(dt_of(qkv), qkv.data_ptr(), o.data_ptr(), lse.data_ptr<float>(), dout.data_ptr(),
                             dqkv.data_ptr(), delta.data_ptr<float>(), opt_ptr<float>(&dkv_part), cu.data_ptr<int>(),
                             pos_ids.data_ptr<int>(), N, n.B, n.T, n.H, n.G, n.hd, rcos, rsin, stream());
  return dqkv;
}

// ------------------------------------------------------------------ loss
// logits may be a row-strided view (unit stride within a row): the vocabulary padded to whole
// GEMM tiles in the fused head, CE over the first V columns; one workgroup per row
void ce_logits(const Op& op, const Tensor& logits) {
  op.floating(logits, "logits");
  op.rows(logits, -1, -1, logits.scalar_type(), "logits", false, logits.element_size());
  op.to_int(logits.size(0), "N");
}

std::tuple<Tensor, Tensor> ce_fwd(const Tensor& logits, const Tensor& targets, int64_t ignore_index) {
  Op op("ce_fwd", logits, "logits");
  ce_logits(op, logits);
  const int64_t N = logits.size(0), V = logits.size(1);
  op.shaped(targets, {N}, at::kLong, "targets");
  auto loss = at::empty({N}, logits.options().dtype(at::kFloat));
  auto lse = at::empty({N}, logits.options().dtype(at::kFloat));
  bllm::ce_fwd(dt_of(logits), logits.data_ptr(), targets.data_ptr<int64_t>(), loss.data_ptr<float>(),
               lse.data_ptr<float>(), N, V, logits.stride(0), ignore_index, stream());
  return {loss, lse};
}

void ce_bwd_(Tensor& logits, const Tensor& targets, const Tensor& lse, const Tensor& scale, int64_t ignore_index) {
  Op op("ce_bwd_", logits, "logits");
  ce_logits(op, logits);
  const int64_t N = logits.size(0), V = logits.size(1);
  op.vec(targets, N, at::kLong, "targets");
  op.vec(lse, N, at::kFloat, "lse");
  op.contig(scale, "scale");
  TORCH_CHECK(scale.scalar_type() == at::kFloat && scale.numel() >= 1, "ce_bwd_: scale must hold one fp32 value");
  bllm::ce_bwd(dt_of(logits), logits.data_ptr(), targets.data_ptr<int64_t>(), lse.data_ptr<float>(),
               scale.data_ptr<float>(), N, V, logits.stride(0), ignore_index, stream());
}

// ------------------------------------------------------------------ embedding
Tensor embedding_fwd(const Tensor& idx, const Tensor& wte, const optional<Tensor>& wpe, int64_t T, double p,
                     int64_t seed, int64_t offset) {
  Op op("embedding_fwd", wte, "wte");
  op.dense(wte, "wte");
  op.dims(wte, 2, "wte");
  op.vec(idx, idx.numel(), at::kLong, "idx");
  const int64_t N = idx.numel();
  const int d = op.to_int(wte.size(1), "d");
  const Tensor* pe = opt(wpe);
  if (pe) {  // position r % T of row r
    op.shaped(*pe, {-1, d}, wte.scalar_type(), "wpe");
    TORCH_CHECK(T > 0 && pe->size(0) >= T && N % T == 0, "embedding_fwd: T = ", T, " must be positive, divide ", N,
                " tokens and fit wpe's ", pe->size(0), " rows");
  }
  auto out = at::empty({N, d}, wte.options());
  bllm::embedding_fwd(dt_of(wte), idx.data_ptr<int64_t>(), wte.data_ptr(), opt_ptr(pe), out.data_ptr(), N, d,
                      op.to_int(T, "T"), (float)p, (uint64_t)seed, (uint64_t)offset, (long)wte.size(0), stream());
  return out;
}

void embedding_bwd(const Tensor& idx, const Tensor& dx, const optional<Tensor>& grad_wte,
                   const optional<Tensor>& grad_wpe, int64_t T, bool accumulate) {
  Op op("embedding_bwd", dx, "dx");
  op.dense(dx, "dx");
  op.dims(dx, 2, "dx");
  const int64_t N = dx.size(0);
  const int d = op.to_int(dx.size(1), "d");
  op.vec(idx, N, at::kLong, "idx");
  if (grad_wte.has_value()) op.shaped(*grad_wte, {-1, d}, dx.scalar_type(), "grad_wte");
  if (grad_wpe.has_value()) {
    op.shaped(*grad_wpe, {-1, d}, dx.scalar_type(), "grad_wpe");
    TORCH_CHECK(T > 0 && N % T == 0 && grad_wpe->size(0) >= T, "embedding_bwd: T = ", T, " must be positive, divide ",
                N, " tokens and fit grad_wpe's ", grad_wpe->size(0), " rows");
  }
  if (grad_wte.has_value()) {
    Tensor gw = *grad_wte;
    if (!accumulate) gw.zero_();
    // stable: equal ids keep their token order, so the fp32 sums run in a fixed order
    auto sorted = at::sort(idx.reshape({-1}), /*stable=*/true, 0, false);
    Tensor sid = std::get<0>(sorted).contiguous(), perm = std::get<1>(sorted).contiguous();
    auto part = at::empty({bllm::embedding_bwd_part_floats(N, d)}, dx.options().dtype(at::kFloat));
    bllm::embedding_bwd_tok(dt_of(dx), sid.data_ptr<int64_t>(), perm.data_ptr<int64_t>(), dx.data_ptr(),
                            gw.data_ptr(), part.data_ptr<float>(), N, d, accumulate, stream());
  }
  if (grad_wpe.has_value()) {
    Tensor gp = *grad_wpe;
    if (!accumulate && gp.size(0) > T) gp.zero_();
    bllm::embedding_bwd_pos(dt_of(dx), dx.data_ptr(), gp.data_ptr(), op.to_int(N / T, "B"), op.to_int(T, "T"), d,
                            accumulate, stream());
  }
}

// ------------------------------------------------------------------ LoRA (csrc/lora.hip)
// out[:, ocol_i : ocol_i + r_i] = scale * x[:, c0_i : c0_i + len_i] . w_i^T ;  w_i [r_i, >= len_i]
void lora_down_impl(const Op& op, const Tensor& x, at::TensorList ws, at::IntArrayRef c0, at::IntArrayRef lens,
                    at::IntArrayRef ocol, int64_t R, double scale, Tensor& out) {
  op.half_only(x, "x");
  op.rows(x, -1, -1, x.scalar_type(), "x");
  const int N = op.to_int(x.size(0), "N");
  TORCH_CHECK(N > 0 && R % 16 == 0 && R > 0, op.name, ": N > 0 and R a multiple of 16 required, got ", N, ", ", R);
  TORCH_CHECK(ws.size() == c0.size() && ws.size() == lens.size() && ws.size() == ocol.size(), op.name,
              ": ws, c0, lens and ocol must have one entry per member");
  op.rows(out, N, R, x.scalar_type(), "out", /*at_least=*/true, out.element_size());
  bllm::LoraDownArgs a{};
  a.x = x.data_ptr(); a.ldx = x.stride(0); a.out = out.data_ptr(); a.ldo = out.stride(0); a.scale = (float)scale;
  a.R = op.to_int(R, "R"); a.zpad = op.to_int(out.size(1) - R, "pad");  // columns past R: zeros (alignment pad)
  for (size_t i = 0; i < ws.size(); ++i) {
    const Tensor& w = ws[i];
    op.rows(w, -1, lens[i], x.scalar_type(), "w", /*at_least=*/true);
    const int64_t r = w.size(0);
    TORCH_CHECK(r % 16 == 0 && lens[i] > 0 && lens[i] % 32 == 0 && c0[i] >= 0 && c0[i] % 8 == 0, op.name,
                ": rank % 16, len % 32, c0 % 8 required, got ", r, ", ", lens[i], ", ", c0[i]);
    TORCH_CHECK(c0[i] + lens[i] <= x.size(1) && ocol[i] >= 0 && ocol[i] + r <= R && ocol[i] % 8 == 0, op.name,
                ": window out of range (c0 ", c0[i], " len ", lens[i], " ocol ", ocol[i], " rank ", r, ")");
    for (int64_t off = 0; off < r; off += 64) {
      TORCH_CHECK(a.n < bllm::LORA_MAX, op.name, ": too many rank chunks");
      a.c0[a.n] = op.to_int(c0[i]); a.len[a.n] = op.to_int(lens[i]); a.ocol[a.n] = op.to_int(ocol[i] + off);
      a.nt[a.n] = op.to_int(std::min<int64_t>(64, r - off) / 16);
      a.w[a.n] = (const char*)w.data_ptr() + off * w.stride(0) * w.element_size();
      a.ldw[a.n] = w.stride(0);
      ++a.n;
    }
  }
  bllm::lora_down(dt_of(x), a, N, stream());
}

Tensor lora_down(const Tensor& x, at::TensorList ws, at::IntArrayRef c0, at::IntArrayRef lens,
                 at::IntArrayRef ocol, int64_t R, double scale) {
  Op op("lora_down", x, "x");
  op.dims(x, 2, "x");
  TORCH_CHECK(R > 0, "lora_down: R must be positive, got ", R);
  auto out = at::empty({x.size(0), R}, x.options());
  lora_down_impl(op, x, ws, c0, lens, ocol, R, scale, out);
  return out;
}

// writes into a row-strided view, e.g. the s t columns of a K-augmented [x | s t] operand
void lora_down_into_(const Tensor& x, at::TensorList ws, at::IntArrayRef c0, at::IntArrayRef lens,
                     at::IntArrayRef ocol, int64_t R, double scale, Tensor& out) {
  Op op("lora_down_into_", x, "x");
  lora_down_impl(op, x, ws, c0, lens, ocol, R, scale, out);
}

// dst [rows, R] (any strides, one of them 1): member i's B_i^T [len_i, r_i] at rows c0_i.., columns
// off_i.., zeros elsewhere -- the B block of a K-augmented LoRA weight, one launch per group
void lora_block_(Tensor& dst, at::TensorList bs, at::IntArrayRef c0, at::IntArrayRef off) {
  Op op("lora_block_", dst, "dst");
  op.half_only(dst, "dst");
  TORCH_CHECK(dst.dim() == 2 && (dst.stride(0) == 1 || dst.stride(1) == 1), "lora_block_: dst is 2-D, one stride 1");
  TORCH_CHECK(bs.size() == c0.size() && bs.size() == off.size() && (int64_t)bs.size() <= bllm::LORA_MAX,
              "lora_block_: bs, c0 and off must have one entry per member, at most ", bllm::LORA_MAX);
  bllm::LoraBlockArgs a{};
  a.dst = dst.data_ptr(); a.s_row = dst.stride(0); a.s_j = dst.stride(1);
  a.rows = op.to_int(dst.size(0), "rows"); a.R = op.to_int(dst.size(1), "R"); a.n = op.to_int(bs.size());
  for (size_t i = 0; i < bs.size(); ++i) {
    const Tensor& b = bs[i];
    op.rows(b, -1, -1, dst.scalar_type(), "B", false, b.element_size());
    TORCH_CHECK(c0[i] >= 0 && off[i] >= 0 && c0[i] + b.size(1) <= dst.size(0) && off[i] + b.size(0) <= dst.size(1),
                "lora_block_: block out of range (c0 ", c0[i], " off ", off[i], " B ", b.sizes(), ")");
    a.c0[i] = op.to_int(c0[i]); a.len[i] = op.to_int(b.size(1)); a.off[i] = op.to_int(off[i]);
    a.r[i] = op.to_int(b.size(0)); a.b[i] = b.data_ptr(); a.ldb[i] = b.stride(0);
  }
  bllm::lora_block(dt_of(dst), a, stream());
}

// y[:, c0_i : c0_i + len_i] = base + bias + scale * t[:, toff_i : toff_i + r_i] . u_i ;  u_i [r_i, len_i], any
// strides; base (same shape as y, may be y itself) and bias ([y.size(1)]) are optional
void lora_up_(Tensor& y, const Tensor& t, at::TensorList us, at::IntArrayRef c0, at::IntArrayRef toff, double scale,
              const optional<Tensor>& base_, const optional<Tensor>& bias_) {
  Op op("lora_up_", y, "y");
  op.half_only(y, "y");
  op.rows(y, -1, -1, y.scalar_type(), "y");
  const int N = op.to_int(y.size(0), "N");
  TORCH_CHECK(N > 0, "lora_up_: y has no rows");
  op.rows(t, N, -1, y.scalar_type(), "t");
  TORCH_CHECK(us.size() == c0.size() && us.size() == toff.size() && (int64_t)us.size() <= bllm::LORA_MAX,
              "lora_up_: us, c0 and toff must have one entry per member, at most ", bllm::LORA_MAX);
  bllm::LoraUpArgs a{};
  a.y = y.data_ptr(); a.ldy = y.stride(0); a.t = t.data_ptr(); a.ldt = t.stride(0); a.scale = (float)scale;
  if (const Tensor* base = opt(base_)) {
    op.rows(*base, N, y.size(1), y.scalar_type(), "base");
    a.base = base->data_ptr(); a.ldb = base->stride(0);
  }
  if (const Tensor* bias = opt(bias_)) {
    op.vec(*bias, y.size(1), y.scalar_type(), "bias");
    TORCH_CHECK(aligned(*bias, 16), "lora_up_: bias must be 16-B aligned");
    a.bias = bias->data_ptr();
  }
  int max_len = 0;
  for (size_t i = 0; i < us.size(); ++i) {
    const Tensor& u = us[i];
    op.on_gpu(u, "u");
    op.dtype(u, y.scalar_type(), "u");
    op.dims(u, 2, "u");
    const int64_t r = u.size(0), len = u.size(1);
    TORCH_CHECK(r % 16 == 0 && r <= 256 && toff[i] >= 0 && toff[i] % 8 == 0 && toff[i] + r <= t.size(1),
                "lora_up_: rank window out of range (rank ", r, " toff ", toff[i], ")");
    TORCH_CHECK(c0[i] >= 0 && c0[i] % 8 == 0 && len % 8 == 0 && c0[i] + len <= y.size(1),
                "lora_up_: output window out of range (c0 ", c0[i], " len ", len, ")");
    a.c0[a.n] = op.to_int(c0[i]); a.len[a.n] = op.to_int(len); a.toff[a.n] = op.to_int(toff[i]);
    a.r[a.n] = op.to_int(r); a.u[a.n] = u.data_ptr(); a.su_j[a.n] = u.stride(0); a.su_c[a.n] = u.stride(1);
    max_len = std::max(max_len, a.len[a.n]);
    ++a.n;
  }
  bllm::lora_up(dt_of(y), a, N, max_len, stream());
}

// g_i[a][b] (+)= scale * sum_n p[n][pa_i + a] * q[n][qb_i + b] ;  g_i [r_i, len_i] view of a contiguous block
void lora_wgrad(const Tensor& p, const Tensor& q, at::TensorList gs, at::IntArrayRef pa, at::IntArrayRef qb,
                double scale, bool accumulate) {
  Op op("lora_wgrad", p, "p");
  op.half_only(p, "p");
  op.rows(p, -1, -1, p.scalar_type(), "p");
  const int N = op.to_int(p.size(0), "N");
  TORCH_CHECK(N > 0, "lora_wgrad: p has no rows");
  op.rows(q, N, -1, p.scalar_type(), "q");
  TORCH_CHECK(gs.size() == pa.size() && gs.size() == qb.size() && (int64_t)gs.size() <= bllm::LORA_MAX && !gs.empty(),
              "lora_wgrad: gs, pa and qb must have one entry per member, 1 to ", bllm::LORA_MAX);
  bllm::LoraWgradArgs a{};
  a.p = p.data_ptr(); a.ldp = p.stride(0); a.q = q.data_ptr(); a.ldq = q.stride(0);
  a.scale = (float)scale; a.accumulate = accumulate;
  const int64_t esz = gs[0].element_size();
  int blocks = 0;
  for (size_t i = 0; i < gs.size(); ++i) {
    const Tensor& gm = gs[i];
    op.dims(gm, 2, "grad");
    const int64_t r = gm.size(0), len = gm.size(1);
    op.grad_block(gm, r, len, "grad");
    op.dtype(gm, gs[0].scalar_type(), "grad");
    TORCH_CHECK(r % 16 == 0 && r <= 64 && len % 8 == 0 && pa[i] >= 0 && pa[i] % 8 == 0 && qb[i] >= 0 && qb[i] % 8 == 0,
                "lora_wgrad: rank % 16 (<= 64), len % 8, pa % 8, qb % 8 required, got ", r, ", ", len, ", ", pa[i],
                ", ", qb[i]);
    TORCH_CHECK(pa[i] + r <= p.size(1) && qb[i] + len <= q.size(1), "lora_wgrad: window out of range (pa ", pa[i],
                " qb ", qb[i], " grad ", gm.sizes(), ")");
    // merge into the previous member when both read the same Q window, their P windows are
    // adjacent, their output strides agree and the merged rank stays <= 64 (dA of a group)
    if (a.n > 0) {
      const int j = a.n - 1;
      if (a.qb[j] == qb[i] && a.len[j] == len && a.pa[j] + a.r[j] == pa[i] && a.r[j] + r <= 64 &&
          a.sa[j] == gm.stride(0) && a.sb[j] == gm.stride(1)) {
        for (int64_t t = 0; t < r / 16; ++t)
          a.gt[j][a.r[j] / 16 + t] = (char*)gm.data_ptr() + 16 * t * gm.stride(0) * esz;
        a.r[j] += op.to_int(r);
        continue;
      }
    }
    a.pa[a.n] = op.to_int(pa[i]); a.qb[a.n] = op.to_int(qb[i]); a.r[a.n] = op.to_int(r); a.len[a.n] = op.to_int(len);
    a.nblk[a.n] = bllm::ceil_div(len, 64); a.sa[a.n] = gm.stride(0); a.sb[a.n] = gm.stride(1);
    for (int64_t t = 0; t < r / 16; ++t) a.gt[a.n][t] = (char*)gm.data_ptr() + 16 * t * gm.stride(0) * esz;
    ++a.n;
  }
  for (int i = 0; i < a.n; ++i) blocks += a.nblk[i];
  const int S = bllm::lora_wgrad_splits(blocks, N);
  Tensor part;
  if (S > 1) {
    int64_t total = 0;
    for (int i = 0; i < a.n; ++i) { a.part_off[i] = total; total += (int64_t)a.len[i] * a.r[i]; }
    part = at::empty({S, total}, p.options().dtype(at::kFloat));
    a.part = part.data_ptr<float>(); a.part_ld = total;
  }
  bllm::lora_wgrad(dt_of(p), dt_of(gs[0]), a, N, S, stream());
}

// LoRA head backward of one logits-gradient chunk dl [R, V]: u = dl B^T (written to u [R, 16]) and
// gB (+)= st^T dl (gB [16, V], or a transposed view of a [V, 16] block) in one pass over dl
void lora_head_bwd_(const Tensor& dl, const Tensor& st, const Tensor& B, Tensor& u, Tensor& gB, bool accumulate) {
  Op op("lora_head_bwd_", dl, "dl");
  op.half_only(dl, "dl");
  op.contig(dl, "dl");
  op.dims(dl, 2, "dl");
  const int R = op.to_int(dl.size(0), "R"), V = op.to_int(dl.size(1), "V");
  TORCH_CHECK(V % 64 == 0, "lora_head_bwd_: V must be a multiple of 64, got ", V);
  op.rows(dl, R, V, dl.scalar_type(), "dl");
  op.contig(B, "B");
  op.rows(B, 16, V, dl.scalar_type(), "B");
  op.rows(st, R, 16, dl.scalar_type(), "st");
  op.shaped(u, {R, 16}, dl.scalar_type(), "u");
  op.grad_block(gB, 16, V, "gB");
  const int S = bllm::lora_head_bwd_splits(R, V, dl.stride(0));
  const int64_t slabs = (V + 1023) / 1024;
  auto gpart = at::empty({S, 16 * (int64_t)V}, dl.options().dtype(at::kFloat));
  auto upart = at::empty({slabs, (int64_t)R * 16}, dl.options().dtype(at::kFloat));
  bllm::lora_head_bwd(dt_of(dl), dl.data_ptr(), dl.stride(0), st.data_ptr(), st.stride(0), B.data_ptr(), B.stride(0),
                      gpart.data_ptr<float>(), upart.data_ptr<float>(), u.data_ptr(), R, V, S, stream());
  bllm::LoraWgradArgs a{};
  a.accumulate = accumulate;
  a.n = 1;
  a.r[0] = 16; a.len[0] = V; a.sa[0] = gB.stride(0); a.sb[0] = gB.stride(1);
  a.gt[0][0] = gB.data_ptr();
  a.part_off[0] = 0;
  a.part = gpart.data_ptr<float>(); a.part_ld = 16 * (int64_t)V;
  bllm::lora_reduce(dt_of(gB), a, S, stream());
}

// [R, K] = concat_i a_i^T  (a_i [K, r_i] contiguous)
Tensor lora_pack_t(at::TensorList as) {
  TORCH_CHECK(!as.empty() && (int64_t)as.size() <= bllm::LORA_MAX, "lora_pack_t: 1 to ", bllm::LORA_MAX, " matrices");
  Op op("lora_pack_t", as[0], "a[0]");
  op.floating(as[0], "a[0]");
  op.dims(as[0], 2, "a[0]");
  const int K = op.to_int(as[0].size(0), "K");
  bllm::LoraPackArgs a{};
  int64_t R = 0;
  int max_r = 0;
  for (auto& t : as) {
    op.shaped(t, {K, -1}, as[0].scalar_type(), "a[i]");
    const int r = op.to_int(t.size(1), "rank");
    a.off[a.n] = op.to_int(R, "R"); a.r[a.n] = r; a.a[a.n] = t.data_ptr();
    R += r;
    max_r = std::max(max_r, r);
    ++a.n;
  }
  auto out = at::empty({R, K}, as[0].options());
  a.out = out.data_ptr();
  bllm::lora_pack_t(dt_of(as[0]), a, K, max_r, stream());
  return out;
}

// ------------------------------------------------------------------ optimizer
Tensor sq_norm_multi(at::TensorList ts) {
  TORCH_CHECK(!ts.empty(), "sq_norm_multi: no tensors");
  Op op("sq_norm_multi", ts[0], "ts[0]");
  std::vector<int> slots;
  int total = 0;
  for (auto& t : ts) {
    op.dense(t, "ts[i]");
    slots.push_back(bllm::sqsum_slots(t.numel()));
    total = op.to_int((int64_t)total + slots.back(), "the partial count");
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

void adamw_step_(Tensor& param, const optional<Tensor>& master_, const Tensor& grad, Tensor& exp_avg,
                 Tensor& exp_avg_sq, double lr, double b1, double b2, double eps, double wd, int64_t step,
                 const optional<Tensor>& grad_scale_) {
  Op op("adamw_step_", param, "param");
  op.dense(param, "param");
  const int64_t n = param.numel();
  op.floating(grad, "grad");
  op.vec(grad, n, grad.scalar_type(), "grad");
  op.vec(exp_avg, n, at::kFloat, "exp_avg");
  op.vec(exp_avg_sq, n, at::kFloat, "exp_avg_sq");
  const Tensor* master = opt(master_);
  if (master) op.vec(*master, n, at::kFloat, "master");
  const Tensor* grad_scale = opt(grad_scale_);
  if (grad_scale) {
    op.contig(*grad_scale, "grad_scale");
    TORCH_CHECK(grad_scale->scalar_type() == at::kFloat && grad_scale->numel() >= 1,
                "adamw_step_: grad_scale must hold one fp32 value");
  }
  bllm::adamw_step(dt_of(param), dt_of(grad), param.data_ptr(), opt_ptr<float>(master), grad.data_ptr(),
                   exp_avg.data_ptr<float>(), exp_avg_sq.data_ptr<float>(), n, lr, b1, b2, eps, wd,
                   op.to_int(step, "step"), opt_ptr<float>(grad_scale), stream());
}

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

Tensor linear_residual(const Tensor& x, const Tensor& W, const Tensor& C) {
  Op op("linear_residual", x, "x");
  op.half_only(x, "x");
  op.contig(x, "x");
  op.dims(x, 2, "x");
  op.dims(W, 2, "W");
  const int64_t N = x.size(0), K = x.size(1), O = W.size(0);
  op.shaped(W, {O, K}, x.scalar_type(), "W");
  op.shaped(C, {N, O}, x.scalar_type(), "C");
  const int dev = x.get_device();
  TORCH_CHECK(dev >= 0 && dev < 64, "linear_residual: device index ", dev, " outside [0, 64)");
  const hipDataType dt = x.scalar_type() == at::kBFloat16 ? HIP_R_16BF : HIP_R_16F;
  auto D = at::empty({N, O}, x.options());
  auto ws = at::empty({(int64_t)kLtWorkspace}, x.options().dtype(at::kByte));
  const LtPlan& p = lt_plan(dev, dt, N, K, O);
  const float alpha = 1.f, beta = 1.f;
  LT_CHECK(hipblasLtMatmul(lt_handle(dev), p.op, &alpha, W.data_ptr(), p.a, x.data_ptr(), p.b, &beta, C.data_ptr(),
                           p.c, D.data_ptr(), p.c, &p.algo, ws.data_ptr(), kLtWorkspace, stream()));
  return D;
}

// ------------------------------------------------------------------ fp8-weight projection
// y [M, N] = x [M, K] . dequant(pack)^T (+ bias [N]) (+ residual [M, N]) (csrc/linear_w8.hip):
// x bf16 / fp16; packed = the bytes of ops.w8_pack (uint8, N padded to row tiles, times K);
// scale fp32 [N], which also gives N; bias / residual of x's dtype
Tensor linear_w8(const Tensor& x, const Tensor& packed, const Tensor& scale, const optional<Tensor>& bias_,
                 const optional<Tensor>& residual_) {
  Op op("linear_w8", x, "x");
  op.half_only(x, "x");
  op.contig(x, "x");
  op.dims(x, 2, "x");
  op.dims(scale, 1, "scale");
  const int64_t M = x.size(0), K = x.size(1), N = scale.size(0), TN = bllm::linear_w8_row_tile();
  op.vec(scale, N, at::kFloat, "scale");
  const int m = op.to_int(M, "M"), n = op.to_int(N, "N"), k = op.to_int(K, "K");
  TORCH_CHECK(bllm::linear_w8_supported(m, n, k), op.name, ": x ", x.sizes(), " with ", N,
              " output rows: M, N >= 1 and K a positive multiple of ", bllm::linear_w8_k_granule());
  op.vec(packed, (N + TN - 1) / TN * TN * K, at::kByte, "packed");
  const Tensor* bias = opt(bias_);
  const Tensor* res = opt(residual_);
  if (bias) op.vec(*bias, N, x.scalar_type(), "bias");
  if (res) op.shaped(*res, {M, N}, x.scalar_type(), "residual");
  TORCH_CHECK(aligned(x, 16) && aligned(packed, 16) && aligned(scale, 4) && (!res || aligned(*res, 16)), op.name,
              ": x, packed and residual must be 16-byte aligned");
  auto y = at::empty({M, N}, x.options());
  bllm::linear_w8(dt_of(x), x.data_ptr(), packed.data_ptr(), scale.data_ptr<float>(), opt_ptr(bias), opt_ptr(res),
                  y.data_ptr(), m, n, k, stream());
  return y;
}

// ------------------------------------------------------------------ MXFP4-weight projection
// The same on an MXFP4 pack (csrc/linear_w4.hip): packed = the code bytes of ops.w4_pack (uint8, N
// padded to row tiles, times K / 2), scale = its E8M0 bytes (uint8, padded N times K / 32); N is
// passed, since neither length gives it
Tensor linear_w4(const Tensor& x, const Tensor& packed, const Tensor& scale, int64_t N,
                 const optional<Tensor>& bias_, const optional<Tensor>& residual_) {
  Op op("linear_w4", x, "x");
  op.half_only(x, "x");
  op.contig(x, "x");
  op.dims(x, 2, "x");
  const int64_t M = x.size(0), K = x.size(1), TN = bllm::linear_w4_row_tile();
  const int m = op.to_int(M, "M"), n = op.to_int(N, "N"), k = op.to_int(K, "K");
  TORCH_CHECK(bllm::linear_w4_supported(m, n, k) && K <= kMaxGemmPitch, op.name, ": x ", x.sizes(), " with ", N,
              " output rows: M, N >= 1 and K a positive multiple of ", bllm::linear_w4_k_granule(), ", at most ",
              kMaxGemmPitch);
  const int64_t Np = (N + TN - 1) / TN * TN;
  op.vec(packed, Np * K / 2, at::kByte, "packed");
  op.vec(scale, Np * K / 32, at::kByte, "scale");
  const Tensor* bias = opt(bias_);
  const Tensor* res = opt(residual_);
  if (bias) op.vec(*bias, N, x.scalar_type(), "bias");
  if (res) op.shaped(*res, {M, N}, x.scalar_type(), "residual");
  TORCH_CHECK(aligned(x, 16) && aligned(packed, 16) && (!res || aligned(*res, 16)), op.name,
              ": x, packed and residual must be 16-byte aligned");
  auto y = at::empty({M, N}, x.options());
  bllm::linear_w4(dt_of(x), x.data_ptr(), packed.data_ptr(), scale.data_ptr(), opt_ptr(bias), opt_ptr(res),
                  y.data_ptr(), m, n, k, stream());
  return y;
}

// ------------------------------------------------------------------ sampler
// logits [B, V] -> tokens int64 [B]: temperature (0: argmax), top-k (0 or >= V: off), top-p (1: off)
// and a Gumbel-max draw from the counter-based stream (seed, stream[b], ctr[b]) (csrc/sample.hip).
// Step state on the device, for graph replay: the token also goes to next_idx[b], out[b, ctr[b]]
// and (== eos_id; negative: no eos) finished[b]; thr[b] = smallest kept logit; ctr[b] += 1.
// ctr[b] < out.size(1) lives in device memory and cannot be checked here without a sync: the
// generate functions guarantee it by construction (one call per output column), the kernel
// clamps the column it writes, and the kernel-debug build reports a counter outside out.
Tensor sample_rows(const Tensor& logits, const Tensor& streams, Tensor& ctr, int64_t seed, double temperature,
                   int64_t top_k, double top_p, int64_t eos_id, const optional<Tensor>& next_idx,
                   const optional<Tensor>& out, const optional<Tensor>& finished, const optional<Tensor>& thr) {
  Op op("sample_rows", logits, "logits");
  op.dense(logits, "logits");
  op.dims(logits, 2, "logits");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(B > 0 && V > 0, "sample_rows: logits must be a non-empty [B, V], got ", logits.sizes());
  TORCH_CHECK(temperature >= 0.0, "sample_rows: temperature must be >= 0, got ", temperature);   // false for NaN
  TORCH_CHECK(top_k >= 0, "sample_rows: top_k must be >= 0 (0: off), got ", top_k);
  TORCH_CHECK(top_p > 0.0 && top_p <= 1.0, "sample_rows: top_p must be in (0, 1], got ", top_p);
  op.vec(streams, B, at::kLong, "stream");
  op.vec(ctr, B, at::kInt, "ctr");
  const Tensor *ni = opt(next_idx), *o = opt(out), *fin = opt(finished), *th = opt(thr);
  if (ni) op.vec(*ni, B, at::kLong, "next_idx");
  if (o) {   // [B, n >= 1] rows with unit column stride (a column range of a wider buffer is fine)
    op.on_gpu(*o, "out");
    op.dtype(*o, at::kLong, "out");
    TORCH_CHECK(o->dim() == 2 && o->size(0) == B && o->size(1) >= 1 && o->stride(1) == 1 &&
                    (B == 1 || o->stride(0) >= o->size(1)),
                "sample_rows: out must be [", B, ", >= 1] with unit column stride and rows that do not overlap, got ",
                o->sizes(), " strides ", o->strides());
  }
  if (fin) op.vec(*fin, B, at::kBool, "finished");
  if (th) op.vec(*th, B, at::kFloat, "thr");
  auto tokens = at::empty({B}, logits.options().dtype(at::kLong));
  bllm::sample_rows(dt_of(logits), logits.data_ptr(), streams.data_ptr<int64_t>(), ctr.data_ptr<int>(), (uint64_t)seed,
                    (float)temperature, op.to_int(std::min<int64_t>(top_k, INT_MAX), "top_k"), top_p, (long)eos_id,
                    opt_ptr<int64_t>(ni), opt_ptr<int64_t>(o), o ? (long)o->stride(0) : 0L,
                    o ? op.to_int(o->size(1), "out columns") : 0, opt_ptr<unsigned char>(fin), opt_ptr<float>(th),
                    tokens.data_ptr<int64_t>(), op.to_int(B, "B"), op.to_int(V, "V"), stream());
  return tokens;
}

// Speculative decoding bookkeeping (csrc/spec.hip, ops/reference.py:spec_advance): idx / samp int64
// [B, Q]; hist int32 [B, Lh]; h0 / pos / ctr / nsteps int32 [B]; finished bool [B]; out int64 [B, new]
void spec_advance_(Tensor& idx, const Tensor& samp, Tensor& hist, const Tensor& h0, Tensor& pos, Tensor& ctr,
                   Tensor& nsteps, Tensor& finished, Tensor& out, int64_t eos_id, int64_t ngram, bool accept) {
  Op op("spec_advance_", idx, "idx");
  op.dims(idx, 2, "idx");
  const int64_t B = idx.size(0), Q = idx.size(1);
  TORCH_CHECK(B > 0 && bllm::spec_advance_supported((int)std::min<int64_t>(Q, INT_MAX),
                                                    (int)std::clamp<int64_t>(ngram, -1, INT_MAX)),
              "spec_advance_: idx must be [B >= 1, Q in 1..8] and ngram in 1..4, got ", idx.sizes(), " ngram ", ngram);
  op.shaped(idx, {B, Q}, at::kLong, "idx");
  op.contig(idx, "idx");
  op.shaped(samp, {B, Q}, at::kLong, "samp");
  op.contig(samp, "samp");
  op.dims(hist, 2, "hist");
  op.shaped(hist, {B, -1}, at::kInt, "hist");
  op.contig(hist, "hist");
  TORCH_CHECK(hist.size(1) >= 1, "spec_advance_: hist has no columns");
  op.vec(h0, B, at::kInt, "h0");
  op.vec(pos, B, at::kInt, "pos");
  op.vec(ctr, B, at::kInt, "ctr");
  op.vec(nsteps, B, at::kInt, "nsteps");
  op.vec(finished, B, at::kBool, "finished");
  op.on_gpu(out, "out");
  op.dtype(out, at::kLong, "out");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == B && out.size(1) >= 1 && out.stride(1) == 1 &&
                  (B == 1 || out.stride(0) >= out.size(1)),
              "spec_advance_: out must be [", B, ", >= 1] with unit column stride and rows that do not overlap, got ",
              out.sizes(), " strides ", out.strides());
  bllm::spec_advance(idx.data_ptr<int64_t>(), samp.data_ptr<int64_t>(), hist.data_ptr<int>(), h0.data_ptr<int>(),
                     pos.data_ptr<int>(), ctr.data_ptr<int>(), nsteps.data_ptr<int>(),
                     reinterpret_cast<unsigned char*>(finished.data_ptr<bool>()), out.data_ptr<int64_t>(),
                     (long)out.stride(0), op.to_int(B, "B"), (int)Q, op.to_int(hist.size(1), "hist columns"),
                     op.to_int(out.size(1), "out columns"), (long)eos_id, (int)ngram, accept, stream());
}

// ------------------------------------------------------------------ kernel debug mode
// First failed device-side check since the last call (common.h DebugCode; 0 = none), over every
// instrumented translation unit; always 0 in release builds (the checks are compiled away).
int64_t debug_error() {
  const unsigned codes[] = {bllm::debug_take_embedding(), bllm::debug_take_loss(), bllm::debug_take_attn_decode(),
                            bllm::debug_take_attn_decode_split(), bllm::debug_take_attn_decode_fp8(),
                            bllm::debug_take_elementwise(), bllm::debug_take_sample(),
                            bllm::debug_take_attn_extend(), bllm::debug_take_spec()};
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

}  // namespace

// the GPU ops are registered once, schema and HIP ("CUDA" dispatch key) kernel together
#define BLLM_OP(schema, fn) m.def(schema, torch::dispatch(c10::DispatchKey::CUDA, TORCH_FN(fn)))

TORCH_LIBRARY(bllm, m) {
  m.def("debug_error() -> int", &debug_error);
  m.def("set_gemm_tile_maps(int wg_map, int wg_gm, int nt_map, int nt_gm) -> ()", &set_gemm_tile_maps);
  m.def("kernel_debug_build() -> bool", &kernel_debug_build);
  m.def("attn_decode_split_chunk() -> int", &attn_decode_split_chunk);
  BLLM_OP("rmsnorm_fwd(Tensor x, Tensor w, float eps) -> (Tensor, Tensor)", rmsnorm_fwd);
  BLLM_OP("rmsnorm_fwd_into_(Tensor x, Tensor w, float eps, Tensor(a!) y) -> Tensor", rmsnorm_fwd_into_);
  BLLM_OP("rmsnorm_bwd(Tensor dy, Tensor x, Tensor w, Tensor rstd, Tensor? dx_acc, Tensor(a!)? dw_out, bool accumulate) -> (Tensor, Tensor)", rmsnorm_bwd);
  BLLM_OP("layernorm_fwd(Tensor x, Tensor w, Tensor b, float eps) -> (Tensor, Tensor, Tensor)", layernorm_fwd);
  BLLM_OP("layernorm_bwd(Tensor dy, Tensor x, Tensor w, Tensor mean, Tensor rstd, Tensor? dx_acc, Tensor(a!)? dw_out, Tensor(b!)? db_out, bool accumulate) -> (Tensor, Tensor, Tensor)", layernorm_bwd);
  BLLM_OP("dropout_add(Tensor x, Tensor a, float p, int seed, int offset) -> Tensor", dropout_add);
  BLLM_OP("dropout_add_layernorm(Tensor x, Tensor a, Tensor w, Tensor b, float eps, float p, int seed, int offset) -> (Tensor, Tensor, Tensor, Tensor)", dropout_add_layernorm);
  BLLM_OP("dropout_bwd(Tensor dy, float p, int seed, int offset) -> Tensor", dropout_bwd);
  BLLM_OP("bwd_bias_grad_(Tensor(a!) src, Tensor? aux, Tensor(b!)? db, bool accumulate, int op, float p, int seed, int offset, bool act_inplace=False) -> Tensor", bwd_bias_grad_);
  BLLM_OP("transpose2d(Tensor a) -> Tensor", transpose2d);
  BLLM_OP("linear_residual(Tensor x, Tensor W, Tensor C) -> Tensor", linear_residual);
  BLLM_OP("linear_w8(Tensor x, Tensor packed, Tensor scale, Tensor? bias, Tensor? residual) -> Tensor", linear_w8);
  BLLM_OP("linear_w4(Tensor x, Tensor packed, Tensor scale, int N, Tensor? bias, Tensor? residual) -> Tensor",
          linear_w4);
  BLLM_OP("swiglu_fwd(Tensor gu) -> Tensor", swiglu_fwd);
  BLLM_OP("swiglu_fwd_into_(Tensor gu, Tensor(a!) act) -> ()", swiglu_fwd_into_);
  BLLM_OP("swiglu_bwd_lowrank(Tensor gu, Tensor base, Tensor u, Tensor P, float scale) -> Tensor", swiglu_bwd_lowrank);
  BLLM_OP("swiglu_bwd_lowrank_wgrad(Tensor gu, Tensor base, Tensor u, Tensor P, float scale, Tensor st, Tensor(a!) gB_gate, Tensor(b!) gB_up, Tensor(c!) gA_down_t, bool accumulate) -> Tensor", swiglu_bwd_lowrank_wgrad);
  BLLM_OP("lora_head_bwd_(Tensor dl, Tensor st, Tensor B, Tensor(a!) u, Tensor(b!) gB, bool accumulate) -> ()", lora_head_bwd_);
  BLLM_OP("swiglu_bwd(Tensor gu, Tensor dact) -> Tensor", swiglu_bwd);
  BLLM_OP("swiglu_bwd_act(Tensor gu, Tensor(a!) dact) -> Tensor", swiglu_bwd_act);
  BLLM_OP("gelu_fwd(Tensor f) -> Tensor", gelu_fwd);
  BLLM_OP("gelu_bwd(Tensor f, Tensor dg) -> Tensor", gelu_bwd);
  BLLM_OP("rope_(Tensor(a!) qkv, Tensor cos, Tensor sin, int T, int H, int G, int hd, bool inverse, int pos_offset) -> ()", rope_);
  BLLM_OP("bias_grad_(Tensor dy, Tensor(a!) db, bool accumulate) -> ()", bias_grad_);
  BLLM_OP("sum_partials_(Tensor part, Tensor(a!) out, bool accumulate) -> ()", sum_partials_);
  BLLM_OP("wgrad_gemm_(Tensor a, Tensor b, Tensor(a!) c, bool accumulate, int splits) -> ()", wgrad_gemm_);
  BLLM_OP("wgrad_gemm_tail_(Tensor a, Tensor b, Tensor(a!) c, bool accumulate, int full, int St) -> ()", wgrad_gemm_tail_);
  BLLM_OP("gemm_nn_(Tensor a, Tensor b, Tensor(a!) c, bool accumulate) -> ()", gemm_nn_);
  BLLM_OP("gemm_nt_(Tensor a, Tensor b, Tensor(a!) c, bool accumulate) -> ()", gemm_nt_);
  BLLM_OP("gemm_nt_swiglu_(Tensor a, Tensor w, Tensor(a!) gu, Tensor(b!) act) -> ()", gemm_nt_swiglu_);
  BLLM_OP("gemm_nt_rope_(Tensor a, Tensor w, Tensor(a!) qkv, Tensor cos, Tensor sin, int T, int nrot, int hd) -> ()", gemm_nt_rope_);
  BLLM_OP("gemm_nt_bias_gelu_(Tensor a, Tensor w, Tensor bias, Tensor(a!) f, Tensor(b!) g) -> ()", gemm_nt_bias_gelu_);
  BLLM_OP("attn_decode(Tensor q, Tensor kcache, Tensor vcache, int L) -> Tensor", attn_decode);
  BLLM_OP("attn_decode_append(Tensor qkv, Tensor(a!) kcache, Tensor(b!) vcache, Tensor pos, int H, int G) -> Tensor", attn_decode_append);
  BLLM_OP("attn_decode_append_rows(Tensor qkv, Tensor(a!) kcache, Tensor(b!) vcache, Tensor pos, int H, int G) -> Tensor", attn_decode_append_rows);
  BLLM_OP("attn_decode_split(Tensor q, Tensor kcache, Tensor vcache, int L) -> Tensor", attn_decode_split);
  BLLM_OP("attn_decode_append_split(Tensor qkv, Tensor(a!) kcache, Tensor(b!) vcache, Tensor pos, int H, int G) -> Tensor", attn_decode_append_split);
  BLLM_OP("attn_extend_rows(Tensor qkv, Tensor(a!) kcache, Tensor(b!) vcache, Tensor pos, Tensor pos_rows, int Q, int H, int G) -> Tensor", attn_extend_rows);
  BLLM_OP("spec_advance_(Tensor(a!) idx, Tensor samp, Tensor(b!) hist, Tensor h0, Tensor(c!) pos, Tensor(d!) ctr, Tensor(e!) nsteps, Tensor(f!) finished, Tensor(g!) out, int eos_id, int ngram, bool accept) -> ()", spec_advance_);
  BLLM_OP("kv_cache_fill_varlen(Tensor qkv, Tensor cu, Tensor(a!) kcache, Tensor(b!) vcache, Tensor? rows=None) -> ()", kv_cache_fill_varlen);
  BLLM_OP("kv_cache_fill_varlen_fp8(Tensor qkv, Tensor cu, Tensor(a!) kcache, Tensor(b!) kscale, Tensor(c!) vcache, Tensor(d!) vscale, Tensor? rows=None) -> ()", kv_cache_fill_varlen_fp8);
  BLLM_OP("attn_decode_append_rows_fp8(Tensor qkv, Tensor(a!) kcache, Tensor(b!) kscale, Tensor(c!) vcache, Tensor(d!) vscale, Tensor pos, int H, int G) -> Tensor", attn_decode_append_rows_fp8);
  BLLM_OP("rope_dev_(Tensor(a!) qkv, Tensor cos, Tensor sin, int H, int G, int hd, Tensor pos) -> ()", rope_dev_);
  BLLM_OP("rope_pos_(Tensor(a!) qkv, Tensor cos, Tensor sin, Tensor pos_ids, int H, int G, int hd, bool inverse) -> ()", rope_pos_);
  BLLM_OP("flash_attn_varlen_fwd(Tensor qkv, Tensor cu, int max_len, int H, int G, int hd) -> (Tensor, Tensor)", flash_attn_varlen_fwd);
  BLLM_OP("flash_attn_varlen_bwd(Tensor qkv, Tensor o, Tensor lse, Tensor dout, Tensor cu, Tensor pos_ids, int max_len, int H, int G, int hd, Tensor? rope_cos=None, Tensor? rope_sin=None) -> Tensor", flash_attn_varlen_bwd);
  BLLM_OP("flash_attn_fwd(Tensor qkv, int B, int T, int H, int G, int hd, bool causal, float p, int seed, int offset, Tensor(a!)? keep_mask=None) -> (Tensor, Tensor)", flash_attn_fwd);
  BLLM_OP("flash_attn_bwd(Tensor qkv, Tensor o, Tensor lse, Tensor dout, int B, int T, int H, int G, int hd, bool causal, float p, int seed, int offset, Tensor? keep_mask=None, Tensor? rope_cos=None, Tensor? rope_sin=None) -> Tensor", flash_attn_bwd);
  BLLM_OP("ce_fwd(Tensor logits, Tensor targets, int ignore_index) -> (Tensor, Tensor)", ce_fwd);
  BLLM_OP("ce_bwd_(Tensor(a!) logits, Tensor targets, Tensor lse, Tensor scale, int ignore_index) -> ()", ce_bwd_);
  BLLM_OP("sample_rows(Tensor logits, Tensor stream, Tensor(a!) ctr, int seed, float temperature, int top_k, float top_p, int eos_id, Tensor(b!)? next_idx, Tensor(c!)? out, Tensor(d!)? finished, Tensor(e!)? thr) -> Tensor", sample_rows);
  BLLM_OP("embedding_fwd(Tensor idx, Tensor wte, Tensor? wpe, int T, float p, int seed, int offset) -> Tensor", embedding_fwd);
  BLLM_OP("embedding_bwd(Tensor idx, Tensor dx, Tensor(a!)? grad_wte, Tensor(b!)? grad_wpe, int T, bool accumulate) -> ()", embedding_bwd);
  BLLM_OP("lora_down(Tensor x, Tensor[] ws, int[] c0, int[] lens, int[] ocol, int R, float scale) -> Tensor", lora_down);
  BLLM_OP("lora_block_(Tensor(a!) dst, Tensor[] bs, int[] c0, int[] off) -> ()", lora_block_);
  BLLM_OP("lora_down_into_(Tensor x, Tensor[] ws, int[] c0, int[] lens, int[] ocol, int R, float scale, Tensor(a!) out) -> ()", lora_down_into_);
  BLLM_OP("lora_up_(Tensor(a!) y, Tensor t, Tensor[] us, int[] c0, int[] toff, float scale, Tensor? base, Tensor? bias) -> ()", lora_up_);
  BLLM_OP("lora_wgrad(Tensor p, Tensor q, Tensor(a!)[] gs, int[] pa, int[] qb, float scale, bool accumulate) -> ()", lora_wgrad);
  BLLM_OP("lora_pack_t(Tensor[] a) -> Tensor", lora_pack_t);
  BLLM_OP("sq_norm_multi(Tensor[] ts) -> Tensor", sq_norm_multi);
  BLLM_OP("adamw_step_(Tensor(a!) param, Tensor(b!)? master, Tensor grad, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, float lr, float beta1, float beta2, float eps, float wd, int step, Tensor? grad_scale) -> ()", adamw_step_);
}
