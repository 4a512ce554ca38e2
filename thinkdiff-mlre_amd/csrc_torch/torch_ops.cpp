// torch.ops.thinkdiff_hip.* -- the custom-op layer of the MI355X hot path (last row), registered from a
// shared library (lib/libthinkdiff_torch_ops.so, loaded by thinkdiff/ops.py with torch.ops.load_library).
//
// Each op is a schema plus ONE kernel, registered for the "CUDA" (= HIP on ROCm) dispatch key, that hands raw device pointers
// and sizes to the C ABI of libthinkdiff_hip.so (include/thinkdiff_hip.h).  Conventions: tensors are borrowed (caller owns,
// device-resident, innermost stride 1), outputs come from the PyTorch caching allocator on the current HIP stream, nothing
// synchronises, a rejected argument is a TORCH_CHECK failure (Python RuntimeError) carrying td_last_error().  There is no CPU,
// Meta or composite kernel: a call with only host tensors fails in the dispatcher.  The dispatcher picks this kernel as soon as
// ANY argument is on the GPU, so every tensor argument -- the optional ones too -- is checked here for device (all on x's), dtype,
// contiguity and extent before its pointer goes to the C ABI; each op also makes x's device current for its duration (the
// launchers read hipGetDevice() for per-device attributes and their stream-K / split-K workspaces).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <limits>
#include <tuple>

#include "../../include/thinkdiff_hip.h"

namespace {

void* stream_of(const at::Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream(); }
const void* P(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined() ? t->data_ptr() : nullptr; }

void check_rows(const at::Tensor& t, const char* name, at::ScalarType ty = at::kBFloat16) {
  TORCH_CHECK(t.is_cuda(), "thinkdiff_hip: ", name, " must live on the GPU");
  TORCH_CHECK(t.scalar_type() == ty, "thinkdiff_hip: ", name, " has dtype ", t.scalar_type(), ", expected ", ty);
  TORCH_CHECK(t.dim() >= 1 && t.stride(-1) == 1, "thinkdiff_hip: ", name, " needs innermost stride 1");
}
// a per-column / per-row operand: on `like`'s device, dtype `ty`, contiguous, exactly `numel` elements
void check_vec(const at::Tensor& t, const char* name, const at::Tensor& like, int64_t numel, at::ScalarType ty = at::kBFloat16) {
  check_rows(t, name, ty);
  TORCH_CHECK(t.device() == like.device(), "thinkdiff_hip: ", name, " lives on ", t.device(), ", expected ", like.device());
  TORCH_CHECK(t.is_contiguous() && t.numel() == numel, "thinkdiff_hip: ", name, " needs ", numel, " contiguous elements, got ", t.numel());
}
void check_vec(const c10::optional<at::Tensor>& t, const char* name, const at::Tensor& like, int64_t numel, at::ScalarType ty = at::kBFloat16) {
  if (t.has_value() && t->defined()) check_vec(*t, name, like, numel, ty);
}
void same_device(const at::Tensor& t, const char* name, const at::Tensor& like) {
  TORCH_CHECK(t.device() == like.device(), "thinkdiff_hip: ", name, " lives on ", t.device(), ", expected ", like.device());
}
using DeviceGuard = c10::hip::OptionalHIPGuardMasqueradingAsCUDA;
void ok(int rc) { TORCH_CHECK(rc == TD_OK, "libthinkdiff_hip error ", rc, ": ", td_last_error()); }

// y = act(x . w^T + bias) * gate + res      (nn.Linear and its fused neighbours)
at::Tensor linear(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, int64_t act,
                  const c10::optional<at::Tensor>& gate, const c10::optional<at::Tensor>& res) {
  check_rows(x, "x"); check_rows(w, "w"); same_device(w, "w", x);
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && w.is_contiguous() && w.size(1) == x.size(1), "thinkdiff_hip::linear: x [M,K], w [N,K] contiguous");
  check_vec(bias, "bias", x, w.size(0)); check_vec(gate, "gate", x, w.size(0));
  if (res.has_value() && res->defined()) {
    check_rows(*res, "res"); same_device(*res, "res", x);
    TORCH_CHECK(res->dim() == 2 && res->size(0) == x.size(0) && res->size(1) == w.size(0), "thinkdiff_hip::linear: res must be [M,N]");
  }
  DeviceGuard guard(x.device());
  at::Tensor y = at::empty({x.size(0), w.size(0)}, x.options());
  const int64_t ldr = res.has_value() && res->defined() ? res->stride(0) : 0;
  ok(td_linear_bf16(x.data_ptr(), x.stride(0), w.data_ptr(), P(bias), y.data_ptr(), y.stride(0), (int)x.size(0), (int)w.size(0),
                    (int)x.size(1), (int)act, P(gate), P(res), ldr, stream_of(x)));
  return y;
}

// Weight-only e4m3 quantisation with one power-of-two scale per row (td_quant_weight_rows_e4m3): w [N,K] -> (q uint8 [N,K], scale fp32 [N], w_hat bf16 [N,K])
std::tuple<at::Tensor, at::Tensor, at::Tensor> quant_weight_rows_e4m3(const at::Tensor& w) {
  check_rows(w, "w");
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous(), "thinkdiff_hip::quant_weight_rows_e4m3: w [N,K] contiguous");
  DeviceGuard guard(w.device());
  at::Tensor q = at::empty({w.size(0), w.size(1)}, w.options().dtype(at::kByte));
  at::Tensor scale = at::empty({w.size(0)}, w.options().dtype(at::kFloat));
  at::Tensor w_hat = at::empty_like(w);
  ok(td_quant_weight_rows_e4m3(w.data_ptr(), w.stride(0), q.data_ptr(), (float*)scale.data_ptr(), w_hat.data_ptr(), (int)w.size(0), (int)w.size(1), stream_of(w)));
  return std::make_tuple(q, scale, w_hat);
}

// e4m3 KV-cache rows (td_kv_quant_rows_e4m3): kv bf16 [rows, >= heads 128] -> (q uint8 [rows, heads 128], scale fp32 [rows, heads] = 2^e, kv_hat bf16 [rows, heads 128])
std::tuple<at::Tensor, at::Tensor, at::Tensor> kv_quant_rows_e4m3(const at::Tensor& kv, int64_t heads) {
  check_rows(kv, "kv");
  TORCH_CHECK(kv.dim() == 2 && heads > 0 && kv.size(1) == heads * 128 && kv.size(0) > 0, "thinkdiff_hip::kv_quant_rows_e4m3: kv [rows, heads x 128]");
  DeviceGuard guard(kv.device());
  at::Tensor q = at::empty({kv.size(0), heads * 128}, kv.options().dtype(at::kByte));
  at::Tensor scale = at::empty({kv.size(0), heads}, kv.options().dtype(at::kFloat));
  at::Tensor kv_hat = at::empty_strided(kv.sizes(), kv.strides(), kv.options());
  ok(td_kv_quant_rows_e4m3(kv.data_ptr(), kv.stride(0), q.data_ptr(), q.stride(0), (float*)scale.data_ptr(), scale.stride(0), kv_hat.data_ptr(), (int)kv.size(0),
                           (int)heads, nullptr, stream_of(kv)));
  return std::make_tuple(q, scale, kv_hat);
}

// ... and back (td_kv_dequant_rows_e4m3): q uint8 [rows, heads 128], scale fp32 [rows, heads] -> bf16 [rows, heads 128]
at::Tensor kv_dequant_rows_e4m3(const at::Tensor& q, const at::Tensor& scale) {
  check_rows(q, "q", at::kByte); check_rows(scale, "scale", at::kFloat); same_device(scale, "scale", q);
  TORCH_CHECK(q.dim() == 2 && scale.dim() == 2 && q.size(0) > 0 && q.size(0) == scale.size(0) && scale.size(1) > 0 && q.size(1) == scale.size(1) * 128,
              "thinkdiff_hip::kv_dequant_rows_e4m3: q [rows, heads x 128], scale [rows, heads]");
  DeviceGuard guard(q.device());
  at::Tensor out = at::empty({q.size(0), q.size(1)}, q.options().dtype(at::kBFloat16));
  ok(td_kv_dequant_rows_e4m3(q.data_ptr(), q.stride(0), (const float*)scale.data_ptr(), scale.stride(0), out.data_ptr(), out.stride(0), (int)q.size(0), (int)scale.size(1),
                             stream_of(q)));
  return out;
}

// Decode attention over an e4m3 cache (td_attention_decode_kv8): q bf16 [B, Hq 128]; k8 / v8 uint8 [B, Skv, >= Hkv 128] and k_scale / v_scale fp32 [B, Skv, >= Hkv]
// (views of the two planes; k and v share their strides); kv_lens int32 [B] or None -> bf16 [B, Hq 128]
at::Tensor attention_decode_kv8(const at::Tensor& q, const at::Tensor& k8, const at::Tensor& v8, const at::Tensor& k_scale, const at::Tensor& v_scale,
                                const c10::optional<at::Tensor>& kv_lens, int64_t Hq, int64_t Hkv, double scale) {
  check_rows(q, "q"); check_rows(k8, "k8", at::kByte); check_rows(v8, "v8", at::kByte); check_rows(k_scale, "k_scale", at::kFloat); check_rows(v_scale, "v_scale", at::kFloat);
  same_device(k8, "k8", q); same_device(v8, "v8", q); same_device(k_scale, "k_scale", q); same_device(v_scale, "v_scale", q);
  TORCH_CHECK(q.dim() == 2 && k8.dim() == 3 && v8.dim() == 3 && k_scale.dim() == 3 && v_scale.dim() == 3 && Hq > 0 && Hkv > 0 && q.size(1) == Hq * 128,
              "thinkdiff_hip::attention_decode_kv8: q [B, Hq x 128], k8 / v8 [B, Skv, Hkv x 128], k_scale / v_scale [B, Skv, Hkv]");
  const int64_t B = q.size(0), Skv = k8.size(1);
  TORCH_CHECK(k8.size(0) == B && v8.sizes() == k8.sizes() && v8.strides() == k8.strides() && k8.size(2) >= Hkv * 128 && k_scale.size(0) == B && k_scale.size(1) == Skv &&
              k_scale.size(2) >= Hkv && v_scale.sizes() == k_scale.sizes() && v_scale.strides() == k_scale.strides(),
              "thinkdiff_hip::attention_decode_kv8: the k and v planes must share shape and strides, with Skv rows per sequence");
  if (kv_lens.has_value() && kv_lens->defined()) check_vec(*kv_lens, "kv_lens", q, B, at::kInt);
  DeviceGuard guard(q.device());
  at::Tensor o = at::empty({B, Hq * 128}, q.options());
  ok(td_attention_decode_kv8(q.data_ptr(), q.stride(0), q.stride(0), k8.data_ptr(), v8.data_ptr(), k8.stride(1), k8.stride(0), (const float*)k_scale.data_ptr(),
                             (const float*)v_scale.data_ptr(), k_scale.stride(1), k_scale.stride(0), o.data_ptr(), o.stride(0), o.stride(0), (int)B, (int)Skv,
                             (const int*)P(kv_lens), (int)Hq, (int)Hkv, (float)scale, stream_of(q)));
  return o;
}

// linear with the weight given as e4m3 bytes + row scales (the 8-bit weight stream, M <= 64)
at::Tensor linear_w8(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& w_scale, const c10::optional<at::Tensor>& bias, int64_t act,
                     const c10::optional<at::Tensor>& gate, const c10::optional<at::Tensor>& res) {
  check_rows(x, "x"); check_rows(wq, "wq", at::kByte); same_device(wq, "wq", x);
  TORCH_CHECK(x.dim() == 2 && wq.dim() == 2 && wq.is_contiguous() && wq.size(1) == x.size(1), "thinkdiff_hip::linear_w8: x [M,K], wq uint8 [N,K] contiguous");
  check_vec(w_scale, "w_scale", x, wq.size(0), at::kFloat);
  check_vec(bias, "bias", x, wq.size(0)); check_vec(gate, "gate", x, wq.size(0));
  if (res.has_value() && res->defined()) {
    check_rows(*res, "res"); same_device(*res, "res", x);
    TORCH_CHECK(res->dim() == 2 && res->size(0) == x.size(0) && res->size(1) == wq.size(0), "thinkdiff_hip::linear_w8: res must be [M,N]");
  }
  DeviceGuard guard(x.device());
  at::Tensor y = at::empty({x.size(0), wq.size(0)}, x.options());
  const int64_t ldr = res.has_value() && res->defined() ? res->stride(0) : 0;
  ok(td_linear_w8_bf16(x.data_ptr(), x.stride(0), wq.data_ptr(), (const float*)w_scale.data_ptr(), P(bias), y.data_ptr(), y.stride(0), (int)x.size(0),
                       (int)wq.size(0), (int)x.size(1), (int)act, P(gate), P(res), ldr, stream_of(x)));
  return y;
}

// Weight-only MXFP4 quantisation (td_quant_weight_rows_mxfp4): w [N,K] -> (packed uint8 [N,K/2], scales uint8 [N,K/32], w_hat bf16 [N,K])
std::tuple<at::Tensor, at::Tensor, at::Tensor> quant_weight_rows_mxfp4(const at::Tensor& w) {
  check_rows(w, "w");
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous() && w.size(1) % 32 == 0, "thinkdiff_hip::quant_weight_rows_mxfp4: w [N,K] contiguous, K a multiple of 32");
  DeviceGuard guard(w.device());
  at::Tensor packed = at::empty({w.size(0), w.size(1) / 2}, w.options().dtype(at::kByte));
  at::Tensor scales = at::empty({w.size(0), w.size(1) / 32}, w.options().dtype(at::kByte));
  at::Tensor w_hat = at::empty_like(w);
  ok(td_quant_weight_rows_mxfp4(w.data_ptr(), w.stride(0), packed.data_ptr(), scales.data_ptr(), w_hat.data_ptr(), (int)w.size(0), (int)w.size(1), stream_of(w)));
  return std::make_tuple(packed, scales, w_hat);
}

namespace {
// packed uint8 [N,K/2] contiguous with scales uint8 [N,K/32] contiguous on its device
void check_mxfp4(const at::Tensor& packed, const at::Tensor& scales, const char* op) {
  check_rows(packed, "packed", at::kByte); check_rows(scales, "scales", at::kByte); same_device(scales, "scales", packed);
  TORCH_CHECK(packed.dim() == 2 && packed.is_contiguous() && scales.dim() == 2 && scales.is_contiguous() && packed.size(0) > 0 && packed.size(1) % 16 == 0 &&
                  scales.size(0) == packed.size(0) && scales.size(1) * 16 == packed.size(1),
              "thinkdiff_hip::", op, ": packed uint8 [N,K/2] and scales uint8 [N,K/32], both contiguous, K a multiple of 32");
}
}  // namespace

// ... and back (td_dequant_rows_mxfp4): packed, scales -> bf16 [N,K]
at::Tensor dequant_rows_mxfp4(const at::Tensor& packed, const at::Tensor& scales) {
  check_mxfp4(packed, scales, "dequant_rows_mxfp4");
  DeviceGuard guard(packed.device());
  at::Tensor w_hat = at::empty({packed.size(0), packed.size(1) * 2}, packed.options().dtype(at::kBFloat16));
  ok(td_dequant_rows_mxfp4(packed.data_ptr(), scales.data_ptr(), w_hat.data_ptr(), w_hat.stride(0), (int)packed.size(0), (int)packed.size(1) * 2, stream_of(packed)));
  return w_hat;
}

// linear with the weight given as MXFP4 nibbles + block scale bytes (the 4-bit weight stream, M <= 64)
at::Tensor linear_w4(const at::Tensor& x, const at::Tensor& packed, const at::Tensor& scales, const c10::optional<at::Tensor>& bias, int64_t act,
                     const c10::optional<at::Tensor>& gate, const c10::optional<at::Tensor>& res) {
  check_rows(x, "x"); same_device(packed, "packed", x);
  check_mxfp4(packed, scales, "linear_w4");
  TORCH_CHECK(x.dim() == 2 && packed.size(1) * 2 == x.size(1), "thinkdiff_hip::linear_w4: x [M,K], packed uint8 [N,K/2]");
  check_vec(bias, "bias", x, packed.size(0)); check_vec(gate, "gate", x, packed.size(0));
  if (res.has_value() && res->defined()) {
    check_rows(*res, "res"); same_device(*res, "res", x);
    TORCH_CHECK(res->dim() == 2 && res->size(0) == x.size(0) && res->size(1) == packed.size(0), "thinkdiff_hip::linear_w4: res must be [M,N]");
  }
  DeviceGuard guard(x.device());
  at::Tensor y = at::empty({x.size(0), packed.size(0)}, x.options());
  const int64_t ldr = res.has_value() && res->defined() ? res->stride(0) : 0;
  ok(td_linear_w4_bf16(x.data_ptr(), x.stride(0), packed.data_ptr(), scales.data_ptr(), P(bias), y.data_ptr(), y.stride(0), (int)x.size(0),
                       (int)packed.size(0), (int)x.size(1), (int)act, P(gate), P(res), ldr, stream_of(x)));
  return y;
}

namespace {
// packed uint8 [N,K/2], scales fp16 [N,K/G], zeros uint8 [N,K/G], all contiguous on one device, G one of 32 / 64 / 128
void check_int4(const at::Tensor& packed, const at::Tensor& scales, const at::Tensor& zeros, int64_t G, const char* op) {
  check_rows(packed, "packed", at::kByte); check_rows(scales, "scales", at::kHalf); check_rows(zeros, "zeros", at::kByte);
  same_device(scales, "scales", packed); same_device(zeros, "zeros", packed);
  TORCH_CHECK(G == 32 || G == 64 || G == 128, "thinkdiff_hip::", op, ": group_size ", G, " is not one of 32, 64, 128");
  const int64_t K = packed.dim() == 2 ? packed.size(1) * 2 : 0;
  TORCH_CHECK(packed.dim() == 2 && packed.is_contiguous() && scales.dim() == 2 && scales.is_contiguous() && zeros.dim() == 2 && zeros.is_contiguous() &&
                  packed.size(0) > 0 && K > 0 && K % G == 0 && K % 32 == 0 && scales.size(0) == packed.size(0) && scales.size(1) == K / G &&
                  zeros.size(0) == packed.size(0) && zeros.size(1) == K / G,
              "thinkdiff_hip::", op, ": packed uint8 [N,K/2], scales float16 [N,K/G] and zeros uint8 [N,K/G], all contiguous, K a multiple of G and of 32");
}
}  // namespace

// One AWQ (layout 0) / GPTQ (1; 3 = gptq_v2) checkpoint Linear -> (packed uint8 [N,K/2], scales float16 [N,K/G], zeros uint8 [N,K/G]) (td_repack_int4)
std::tuple<at::Tensor, at::Tensor, at::Tensor> repack_int4(int64_t layout, const at::Tensor& qweight, const at::Tensor& qzeros, const at::Tensor& scales, int64_t G) {
  check_rows(qweight, "qweight", at::kInt); check_rows(qzeros, "qzeros", at::kInt); check_rows(scales, "scales", at::kHalf);
  same_device(qzeros, "qzeros", qweight); same_device(scales, "scales", qweight);
  TORCH_CHECK(layout == 0 || layout == 1 || layout == 3, "thinkdiff_hip::repack_int4: layout ", layout, " is not 0 (AWQ), 1 (GPTQ) or 3 (GPTQ v2)");
  TORCH_CHECK(G == 32 || G == 64 || G == 128, "thinkdiff_hip::repack_int4: group_size ", G, " is not one of 32, 64, 128");
  TORCH_CHECK(qweight.dim() == 2 && qweight.is_contiguous() && qzeros.dim() == 2 && qzeros.is_contiguous() && scales.dim() == 2 && scales.is_contiguous(),
              "thinkdiff_hip::repack_int4: qweight, qzeros and scales must be contiguous matrices");
  const int64_t K = layout == 0 ? qweight.size(0) : qweight.size(0) * 8, N = layout == 0 ? qweight.size(1) * 8 : qweight.size(1);
  TORCH_CHECK(N > 0 && K > 0 && N % 8 == 0 && K % G == 0 && K % 32 == 0 && qzeros.size(0) == K / G && qzeros.size(1) == N / 8 && scales.size(0) == K / G && scales.size(1) == N,
              "thinkdiff_hip::repack_int4: qzeros must be int32 [K/G,N/8] and scales float16 [K/G,N] for the N=", N, ", K=", K, " of qweight");
  DeviceGuard guard(qweight.device());
  at::Tensor packed = at::empty({N, K / 2}, qweight.options().dtype(at::kByte));
  at::Tensor s_out = at::empty({N, K / G}, qweight.options().dtype(at::kHalf));
  at::Tensor z_out = at::empty({N, K / G}, qweight.options().dtype(at::kByte));
  ok(td_repack_int4((int)layout, qweight.data_ptr(), qzeros.data_ptr(), scales.data_ptr(), nullptr, (int)N, (int)K, (int)G, packed.data_ptr(), s_out.data_ptr(),
                    z_out.data_ptr(), stream_of(qweight)));
  return std::make_tuple(packed, s_out, z_out);
}

// packed, scales, zeros -> bf16 [N,K] = bf16_rne((q - z) s) (td_dequant_rows_int4)
at::Tensor dequant_rows_int4(const at::Tensor& packed, const at::Tensor& scales, const at::Tensor& zeros, int64_t G) {
  check_int4(packed, scales, zeros, G, "dequant_rows_int4");
  DeviceGuard guard(packed.device());
  at::Tensor w_hat = at::empty({packed.size(0), packed.size(1) * 2}, packed.options().dtype(at::kBFloat16));
  ok(td_dequant_rows_int4(packed.data_ptr(), scales.data_ptr(), zeros.data_ptr(), (int)G, w_hat.data_ptr(), w_hat.stride(0), (int)packed.size(0),
                          (int)packed.size(1) * 2, stream_of(packed)));
  return w_hat;
}

// linear with the weight given as grouped int4 nibbles + fp16 group scales + zero points (the AWQ / GPTQ weight stream, M <= 64)
at::Tensor linear_i4(const at::Tensor& x, const at::Tensor& packed, const at::Tensor& scales, const at::Tensor& zeros, int64_t G,
                     const c10::optional<at::Tensor>& bias, int64_t act, const c10::optional<at::Tensor>& gate, const c10::optional<at::Tensor>& res) {
  check_rows(x, "x"); same_device(packed, "packed", x);
  check_int4(packed, scales, zeros, G, "linear_i4");
  TORCH_CHECK(x.dim() == 2 && packed.size(1) * 2 == x.size(1), "thinkdiff_hip::linear_i4: x [M,K], packed uint8 [N,K/2]");
  check_vec(bias, "bias", x, packed.size(0)); check_vec(gate, "gate", x, packed.size(0));
  if (res.has_value() && res->defined()) {
    check_rows(*res, "res"); same_device(*res, "res", x);
    TORCH_CHECK(res->dim() == 2 && res->size(0) == x.size(0) && res->size(1) == packed.size(0), "thinkdiff_hip::linear_i4: res must be [M,N]");
  }
  DeviceGuard guard(x.device());
  at::Tensor y = at::empty({x.size(0), packed.size(0)}, x.options());
  const int64_t ldr = res.has_value() && res->defined() ? res->stride(0) : 0;
  ok(td_linear_i4_bf16(x.data_ptr(), x.stride(0), packed.data_ptr(), scales.data_ptr(), zeros.data_ptr(), (int)G, P(bias), y.data_ptr(), y.stride(0),
                       (int)x.size(0), (int)packed.size(0), (int)x.size(1), (int)act, P(gate), P(res), ldr, stream_of(x)));
  return y;
}

// ThinkDiff aligner mm_projector "mlp2x_gelu_t5_norm": T5LayerNorm(Linear2(GELU_erf(Linear0(x))))
at::Tensor aligner_mlp2x(const at::Tensor& x, const at::Tensor& w0, const at::Tensor& b0, const at::Tensor& w2, const at::Tensor& b2,
                         const at::Tensor& norm_w, double eps, bool fp32_norm) {
  check_rows(x, "x"); check_rows(w0, "w0"); check_rows(w2, "w2");
  TORCH_CHECK(x.dim() == 2 && w0.dim() == 2 && w2.dim() == 2, "thinkdiff_hip::aligner_mlp2x: x [M,K], w0 [H,K], w2 [H,H]");
  const int64_t M = x.size(0), K = x.size(1), H = w0.size(0);
  check_vec(w0, "w0", x, H * K); check_vec(w2, "w2", x, H * H);
  TORCH_CHECK(w0.size(1) == K && w2.size(0) == H && w2.size(1) == H, "thinkdiff_hip::aligner_mlp2x: w0 must be [H,K] and w2 [H,H]");
  check_vec(b0, "b0", x, H); check_vec(b2, "b2", x, H); check_vec(norm_w, "norm_w", x, H);
  DeviceGuard guard(x.device());
  at::Tensor ws = at::empty({2 * M * H}, x.options());
  at::Tensor y = at::empty({M, H}, x.options());
  ok(td_aligner_mlp2x_bf16(x.data_ptr(), x.stride(0), (int)M, (int)K, (int)H, w0.data_ptr(), b0.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                           norm_w.data_ptr(), (float)eps, fp32_norm ? 1 : 0, ws.data_ptr(), y.data_ptr(), H, stream_of(x)));
  return y;
}

// softmax(q.k^T * scale [+ causal mask]) . v on token-major fused projections: q [B,Sq,>=Hq*128], k/v [B,Skv,>=Hkv*128]
at::Tensor attention(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, int64_t Hq, int64_t Hkv, double scale, bool causal) {
  check_rows(q, "q"); check_rows(k, "k"); check_rows(v, "v");
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3 && k.strides() == v.strides(), "thinkdiff_hip::attention: q/k/v [B,S,cols], k and v with equal strides");
  same_device(k, "k", q); same_device(v, "v", q);
  TORCH_CHECK(Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "thinkdiff_hip::attention: Hq must be a positive multiple of Hkv");
  TORCH_CHECK(q.size(2) >= Hq * 128 && k.size(2) >= Hkv * 128 && v.size(2) >= Hkv * 128,
              "thinkdiff_hip::attention: q needs >= Hq*128 columns and k/v >= Hkv*128 (got ", q.size(2), ", ", k.size(2), ", ", v.size(2), ")");
  TORCH_CHECK(k.size(0) == q.size(0) && v.size(0) == q.size(0) && v.size(1) == k.size(1), "thinkdiff_hip::attention: q/k/v batch sizes and k/v lengths must agree");
  DeviceGuard guard(q.device());
  at::Tensor o = at::empty({q.size(0), q.size(1), Hq * 128}, q.options());
  ok(td_attention_bf16(q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(1), k.stride(0), o.data_ptr(),
                       o.stride(1), o.stride(0), (int)q.size(0), (int)q.size(1), (int)k.size(1), (int)Hq, (int)Hkv, 128, (float)scale,
                       causal ? 1 : 0, stream_of(q)));
  return o;
}

// LayerNorm (no affine) / RMSNorm rows with optional adaLN modulation y*(1+scale)+shift (set A for rows < split, set B after)
at::Tensor norm_rows(const at::Tensor& x, bool rms, double eps, const c10::optional<at::Tensor>& w, int64_t split,
                     const c10::optional<at::Tensor>& shiftA, const c10::optional<at::Tensor>& scaleA,
                     const c10::optional<at::Tensor>& shiftB, const c10::optional<at::Tensor>& scaleB) {
  check_rows(x, "x");
  TORCH_CHECK(x.dim() == 2, "thinkdiff_hip::norm_rows: x [rows,D]");
  const int64_t Dn = x.size(1);
  check_vec(w, "w", x, Dn); check_vec(shiftA, "shiftA", x, Dn); check_vec(scaleA, "scaleA", x, Dn);
  check_vec(shiftB, "shiftB", x, Dn); check_vec(scaleB, "scaleB", x, Dn);
  TORCH_CHECK(split >= 0 && split <= x.size(0), "thinkdiff_hip::norm_rows: split outside [0, rows]");
  DeviceGuard guard(x.device());
  at::Tensor y = at::empty_like(x);
  ok(td_norm_rows_bf16(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), (int)x.size(0), (int)x.size(1), rms ? 1 : 0, (float)eps, P(w),
                       (int)split, P(shiftA), P(scaleA), P(shiftB), P(scaleB), stream_of(x)));
  return y;
}

// in-place per-head RMSNorm(q), RMSNorm(k) + rotary embedding on a fused projection buffer
at::Tensor& qk_norm_rope_(at::Tensor& qkv, int64_t Hq, int64_t Hk, int64_t q_col, int64_t k_col, const at::Tensor& cos, const at::Tensor& sin,
                          int64_t split, const c10::optional<at::Tensor>& wqA, const c10::optional<at::Tensor>& wkA,
                          const c10::optional<at::Tensor>& wqB, const c10::optional<at::Tensor>& wkB, double eps, bool rotate_half) {
  check_rows(qkv, "qkv"); check_rows(cos, "cos", at::kFloat); check_rows(sin, "sin", at::kFloat);
  TORCH_CHECK(qkv.dim() == 2 && cos.is_contiguous() && sin.is_contiguous() && cos.size(0) == qkv.size(0) && cos.size(1) == 128,
              "thinkdiff_hip::qk_norm_rope_: qkv [rows,cols], cos/sin fp32 [rows,128]");
  check_vec(cos, "cos", qkv, qkv.size(0) * 128, at::kFloat); check_vec(sin, "sin", qkv, qkv.size(0) * 128, at::kFloat);
  check_vec(wqA, "wqA", qkv, 128); check_vec(wkA, "wkA", qkv, 128); check_vec(wqB, "wqB", qkv, 128); check_vec(wkB, "wkB", qkv, 128);
  TORCH_CHECK(Hq >= 0 && Hk >= 0 && q_col >= 0 && k_col >= 0 && q_col + Hq * 128 <= qkv.size(1) && k_col + Hk * 128 <= qkv.size(1),
              "thinkdiff_hip::qk_norm_rope_: the q / k head blocks must lie inside a row of qkv");
  TORCH_CHECK(split >= 0 && split <= qkv.size(0), "thinkdiff_hip::qk_norm_rope_: split outside [0, rows]");
  DeviceGuard guard(qkv.device());
  ok(td_qk_norm_rope_bf16(qkv.data_ptr(), qkv.stride(0), (int)qkv.size(0), (int)Hq, (int)Hk, (int)q_col, (int)k_col, (const float*)cos.data_ptr(),
                          (const float*)sin.data_ptr(), (int)split, P(wqA), P(wkA), wqB.has_value() && wqB->defined() ? P(wqB) : P(wqA),
                          wkB.has_value() && wkB->defined() ? P(wkB) : P(wkA), (float)eps, rotate_half ? 1 : 0, stream_of(qkv)));
  return qkv;
}

// FlowMatchEulerDiscreteScheduler.step in place: x = bf16(float(x) + dt * float(v))
at::Tensor& euler_step_(at::Tensor& x, const at::Tensor& v, double dt) {
  check_rows(x, "x"); check_rows(v, "v");
  TORCH_CHECK(x.is_contiguous() && v.is_contiguous() && x.numel() == v.numel(), "thinkdiff_hip::euler_step_: contiguous x, v of equal size");
  same_device(v, "v", x);
  DeviceGuard guard(x.device());
  ok(td_euler_step_bf16(x.data_ptr(), v.data_ptr(), (float)dt, x.numel(), stream_of(x)));
  return x;
}

// FluxKontextPipeline's step under true classifier-free guidance, in place: v = v_neg + scale * (v_pos - v_neg) as three bf16 torch ops with
// the Python float `scale` kept in fp32, then the Euler step (td_flux_cfg_step_bf16)
at::Tensor& flux_cfg_step_(at::Tensor& x, const at::Tensor& v_pos, const at::Tensor& v_neg, double scale, double dt) {
  check_rows(x, "x");
  TORCH_CHECK(x.is_contiguous(), "thinkdiff_hip::flux_cfg_step_: x must be contiguous");
  check_vec(v_pos, "v_pos", x, x.numel()); check_vec(v_neg, "v_neg", x, x.numel());
  DeviceGuard guard(x.device());
  ok(td_flux_cfg_step_bf16(x.data_ptr(), v_pos.data_ptr(), v_neg.data_ptr(), (float)scale, (float)dt, x.numel(), stream_of(x)));
  return x;
}

// FLUX ControlNet residual injection in place: h[:, :D] += bf16(scale * r[:, :D]) with D = r's width, the Python float `scale` kept in fp32
// (td_flux_residual_inject_bf16).  h and r are 2-D views with innermost stride 1: row strides may exceed the width, columns of h beyond D stay.
at::Tensor& flux_residual_inject_(at::Tensor& h, const at::Tensor& r, double scale) {
  check_rows(h, "h"); check_rows(r, "r"); same_device(r, "r", h);
  TORCH_CHECK(h.dim() == 2 && r.dim() == 2 && r.size(0) == h.size(0) && r.size(1) <= h.size(1) && h.size(0) > 0 && r.size(1) > 0,
              "thinkdiff_hip::flux_residual_inject_: h [rows, >= D], r [rows, D] with the same row count");
  DeviceGuard guard(h.device());
  ok(td_flux_residual_inject_bf16(h.data_ptr(), h.stride(0), r.data_ptr(), r.stride(0), (int)h.size(0), (int)r.size(1), (float)scale, stream_of(h)));
  return h;
}

// The same for several ControlNets: h[:, :D] += fold_k bf16(scales[k] * r[k][:, :D]), the fold a bf16 left fold in list order, one launch
// (td_flux_residual_inject_multi_bf16).  1 .. 4 tensors of one width D, each a 2-D view with innermost stride 1 and its own row stride.
at::Tensor& flux_residual_inject_multi_(at::Tensor& h, at::TensorList r, at::ArrayRef<double> scales) {
  check_rows(h, "h");
  TORCH_CHECK(r.size() >= 1 && r.size() <= TD_MAX_CONTROLNETS && r.size() == scales.size(),
              "thinkdiff_hip::flux_residual_inject_multi_: 1 .. ", TD_MAX_CONTROLNETS, " tensors and as many scales, got ", r.size(), " and ", scales.size());
  const void* ptr[TD_MAX_CONTROLNETS];
  int64_t ld[TD_MAX_CONTROLNETS];
  float sc[TD_MAX_CONTROLNETS];
  for (size_t k = 0; k < r.size(); ++k) {
    check_rows(r[k], "r[k]"); same_device(r[k], "r[k]", h);
    TORCH_CHECK(h.dim() == 2 && r[k].dim() == 2 && r[k].size(0) == h.size(0) && r[k].size(1) <= h.size(1) && h.size(0) > 0 && r[k].size(1) > 0 &&
                r[k].size(1) == r[0].size(1), "thinkdiff_hip::flux_residual_inject_multi_: h [rows, >= D], every r[k] [rows, D] with the same row count and width");
    ptr[k] = r[k].data_ptr(); ld[k] = r[k].stride(0); sc[k] = (float)scales[k];
  }
  DeviceGuard guard(h.device());
  ok(td_flux_residual_inject_multi_bf16(h.data_ptr(), h.stride(0), ptr, ld, sc, (int)r.size(), (int)h.size(0), (int)r[0].size(1), stream_of(h)));
  return h;
}

// First-block cache, the residual and its metric sums (td_block_cache_head_bf16): h1, h0 [rows, D] and the optional r_prev, 2-D views with innermost
// stride 1 -> (r = bf16(h1 - h0) [rows, D], sums fp64 [2] = sum |r - r_prev|, sum |r_prev|; both 0 without r_prev).  Deterministic: no atomics.
std::tuple<at::Tensor, at::Tensor> block_cache_head(const at::Tensor& h1, const at::Tensor& h0, const c10::optional<at::Tensor>& r_prev) {
  check_rows(h1, "h1"); check_rows(h0, "h0"); same_device(h0, "h0", h1);
  TORCH_CHECK(h1.dim() == 2 && h0.dim() == 2 && h0.sizes() == h1.sizes() && h1.size(0) > 0 && h1.size(1) > 0, "thinkdiff_hip::block_cache_head: h1, h0 [rows, D] of one shape");
  const bool prev = r_prev.has_value() && r_prev->defined();
  if (prev) {
    check_rows(*r_prev, "r_prev"); same_device(*r_prev, "r_prev", h1);
    TORCH_CHECK(r_prev->dim() == 2 && r_prev->sizes() == h1.sizes(), "thinkdiff_hip::block_cache_head: r_prev must have h1's shape");
  }
  DeviceGuard guard(h1.device());
  at::Tensor r = at::empty({h1.size(0), h1.size(1)}, h1.options());
  at::Tensor sums = at::empty({2}, h1.options().dtype(at::kDouble));
  at::Tensor ws = at::empty({TD_BLOCK_CACHE_WS_BYTES / 8}, h1.options().dtype(at::kDouble));
  ok(td_block_cache_head_bf16(h1.data_ptr(), h1.stride(0), h0.data_ptr(), h0.stride(0), prev ? r_prev->data_ptr() : nullptr, prev ? r_prev->stride(0) : 0, r.data_ptr(),
                              r.stride(0), (int)h1.size(0), (int)h1.size(1), (double*)sums.data_ptr(), ws.data_ptr(), stream_of(h1)));
  return {r, sums};
}
// ... and its tail (td_block_cache_tail_bf16): bf16(a - b) for 2-D views a, b [rows, D] with innermost stride 1
at::Tensor block_cache_tail(const at::Tensor& a, const at::Tensor& b) {
  check_rows(a, "a"); check_rows(b, "b"); same_device(b, "b", a);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.sizes() == b.sizes() && a.size(0) > 0 && a.size(1) > 0, "thinkdiff_hip::block_cache_tail: a, b [rows, D] of one shape");
  DeviceGuard guard(a.device());
  at::Tensor out = at::empty({a.size(0), a.size(1)}, a.options());
  ok(td_block_cache_tail_bf16(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), (int)a.size(0), (int)a.size(1), stream_of(a)));
  return out;
}

// FLUX.1 Redux prompt composition (td_redux_compose_bf16): text [1 or B, T, D] or None (text_rows rows of +0.0), image [B, S, D] or None (S = 0), both
// contiguous, scales B floats (rounded to bf16 by the entry) -> [T + S, D] = sum over b of bf16(s_b * [text[b] | image[b]]), fp32 sum in index order
at::Tensor redux_compose(const c10::optional<at::Tensor>& text, const c10::optional<at::Tensor>& image, at::ArrayRef<double> scales, int64_t text_rows) {
  const bool has_t = text.has_value() && text->defined(), has_i = image.has_value() && image->defined();
  TORCH_CHECK(has_t || has_i, "thinkdiff_hip::redux_compose: text and image are both None");
  const at::Tensor& ref = has_i ? *image : *text;
  const int64_t B = (int64_t)scales.size();
  TORCH_CHECK(B >= 1 && B <= 16, "thinkdiff_hip::redux_compose: ", B, " scales, 1 .. 16 streams are supported");
  check_rows(ref, has_i ? "image" : "text");
  TORCH_CHECK(ref.dim() == 3 && ref.is_contiguous(), "thinkdiff_hip::redux_compose: text / image must be contiguous [batch, rows, D]");
  const int64_t D = ref.size(2);
  if (has_t && has_i) {
    check_rows(*text, "text"); same_device(*text, "text", ref);
    TORCH_CHECK(text->dim() == 3 && text->is_contiguous() && text->size(2) == D, "thinkdiff_hip::redux_compose: text must be contiguous [1 or B, T, ", D, "]");
  }
  TORCH_CHECK(!has_i || image->size(0) == B, "thinkdiff_hip::redux_compose: image has batch ", has_i ? image->size(0) : 0, ", ", B, " scales were given");
  TORCH_CHECK(!has_t || text->size(0) == 1 || text->size(0) == B, "thinkdiff_hip::redux_compose: text has batch ", has_t ? text->size(0) : 0, ", expected 1 or ", B);
  const int64_t T = has_t ? text->size(1) : text_rows, S = has_i ? image->size(1) : 0;
  TORCH_CHECK(T >= 0 && T + S > 0 && T + S < (1ll << 31), "thinkdiff_hip::redux_compose: T = ", T, ", S = ", S, ": T + S must be 1 .. 2^31 - 1");
  float sc[16];
  for (int64_t b = 0; b < B; ++b) sc[b] = (float)scales[b];
  DeviceGuard guard(ref.device());
  at::Tensor out = at::empty({T + S, D}, ref.options());
  ok(td_redux_compose_bf16(has_t ? text->data_ptr() : nullptr, has_t && text->size(0) > 1 ? text->stride(0) : 0, (int)T, has_i ? image->data_ptr() : nullptr,
                           has_i ? image->stride(0) : 0, (int)S, sc, (int)B, (int)D, out.data_ptr(), out.stride(0), stream_of(ref)));
  return out;
}

// FLUX IP-Adapter cross-attention (td_ip_attention_bf16): q [rows, >= H*128] (raw projection rows when norm_w is given: the per-head QK-RMSNorm is
// fused), k / v [n_keys, >= H*128] with equal strides, 1 <= n_keys <= TD_IP_MAX_KEYS -> bf16(out_scale * softmax(qn k^T / sqrt(128)) v) [rows, H*128]
void check_ip(const char* op, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, int64_t H, const c10::optional<at::Tensor>& norm_w) {
  check_rows(q, "q"); check_rows(k, "k"); check_rows(v, "v"); same_device(k, "k", q); same_device(v, "v", q);
  TORCH_CHECK(q.dim() == 2 && k.dim() == 2 && v.dim() == 2 && k.sizes() == v.sizes() && k.strides() == v.strides(), "thinkdiff_hip::", op,
              ": q [rows, cols], k / v [n_keys, cols] with equal shapes and strides");
  TORCH_CHECK(H > 0 && q.size(1) >= H * 128 && k.size(1) >= H * 128, "thinkdiff_hip::", op, ": q and k / v need >= H*128 = ", H * 128, " columns (got ", q.size(1), ", ",
              k.size(1), ")");
  TORCH_CHECK(q.size(0) >= 1 && q.size(0) < (1ll << 31), "thinkdiff_hip::", op, ": q needs 1 .. 2^31 - 1 rows");
  check_vec(norm_w, "norm_w", q, 128);
}
at::Tensor ip_attention(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, int64_t H, const c10::optional<at::Tensor>& norm_w, double eps, double out_scale) {
  check_ip("ip_attention", q, k, v, H, norm_w);
  DeviceGuard guard(q.device());
  at::Tensor o = at::empty({q.size(0), H * 128}, q.options());
  ok(td_ip_attention_bf16(q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0), o.data_ptr(), o.stride(0), (int)q.size(0), (int)H, (int)k.size(0),
                          P(norm_w), (float)eps, (float)out_scale, 0, stream_of(q)));
  return o;
}
// the same into o [rows, >= H*128] (columns beyond H*128 stay); accumulate: o = bf16(o + term), the sum over several adapters
at::Tensor& ip_attention_(at::Tensor& o, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, int64_t H, const c10::optional<at::Tensor>& norm_w, double eps,
                          double out_scale, bool accumulate) {
  check_ip("ip_attention_", q, k, v, H, norm_w);
  check_rows(o, "o"); same_device(o, "o", q);
  TORCH_CHECK(o.dim() == 2 && o.size(0) == q.size(0) && o.size(1) >= H * 128, "thinkdiff_hip::ip_attention_: o must be [rows, >= H*128]");
  DeviceGuard guard(q.device());
  ok(td_ip_attention_bf16(q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0), o.data_ptr(), o.stride(0), (int)q.size(0), (int)H, (int)k.size(0),
                          P(norm_w), (float)eps, (float)out_scale, accumulate ? 1 : 0, stream_of(q)));
  return o;
}
// one parameter of an IP-Adapter slot (td_flux_ip_adapter_load_param; the engine checks the name and the element count)
void flux_ip_adapter_load_param(int64_t engine, int64_t slot, std::string name, const at::Tensor& data) {
  TORCH_CHECK(engine != 0, "thinkdiff_hip: null engine handle");
  check_rows(data, "data");
  TORCH_CHECK(data.is_contiguous(), "thinkdiff_hip::flux_ip_adapter_load_param: '", name, "' must be contiguous");
  DeviceGuard guard(data.device());
  ok(td_flux_ip_adapter_load_param((td_flux*)(uintptr_t)engine, (int)slot, name.c_str(), data.data_ptr(), data.numel(), stream_of(data)));
}
// the image prompt of one image on this context (td_flux_set_ip_image_embeds): embeds [n_img, E] against the slot's embed_dim
void flux_set_ip_image_embeds(int64_t engine, int64_t slot, const at::Tensor& embeds) {
  TORCH_CHECK(engine != 0, "thinkdiff_hip: null engine handle");
  td_flux* f = (td_flux*)(uintptr_t)engine;
  int used = 0, E = 0;
  ok(td_flux_ip_adapter_info(f, (int)slot, &used, nullptr, &E, nullptr, nullptr));
  check_rows(embeds, "embeds");
  TORCH_CHECK(!used || (embeds.dim() == 2 && embeds.is_contiguous() && embeds.size(1) == E && embeds.size(0) >= 1), "thinkdiff_hip::flux_set_ip_image_embeds: slot ", slot,
              " takes contiguous embeds [n_img, ", E, "], got ", embeds.sizes());
  DeviceGuard guard(embeds.device());
  ok(td_flux_set_ip_image_embeds(f, (int)slot, embeds.data_ptr(), embeds.dim() == 2 ? (int)embeds.size(0) : 0, stream_of(embeds)));
}

// FluxInpaintPipeline's step in place: Euler step, scale_noise of the image latents to bf16(sigma_next) (noise None: the clean latents) and
// the mask blend, every op a bf16 torch op (td_flux_inpaint_step_bf16)
at::Tensor& flux_inpaint_step_(at::Tensor& x, const at::Tensor& v, const at::Tensor& image_latents, const c10::optional<at::Tensor>& noise,
                               const at::Tensor& mask, double dt, double sigma_next) {
  check_rows(x, "x");
  TORCH_CHECK(x.is_contiguous(), "thinkdiff_hip::flux_inpaint_step_: x must be contiguous");
  check_vec(v, "v", x, x.numel()); check_vec(image_latents, "image_latents", x, x.numel());
  check_vec(noise, "noise", x, x.numel()); check_vec(mask, "mask", x, x.numel());
  DeviceGuard guard(x.device());
  ok(td_flux_inpaint_step_bf16(x.data_ptr(), v.data_ptr(), image_latents.data_ptr(), P(noise), mask.data_ptr(), (float)dt, (float)sigma_next,
                               x.numel(), stream_of(x)));
  return x;
}

// binarize + F.interpolate(nearest) to (H/8, W/8) + repeat over C channels + _pack_latents: uint8 or float32 [H, W] -> bf16 [(H/16)(W/16), 4C]
at::Tensor flux_inpaint_mask(const at::Tensor& mask, int64_t C) {
  TORCH_CHECK(mask.is_cuda() && mask.is_contiguous() && mask.dim() == 2, "thinkdiff_hip::flux_inpaint_mask: mask must be a contiguous GPU tensor [H, W]");
  const bool u8 = mask.scalar_type() == at::kByte;
  TORCH_CHECK(u8 || mask.scalar_type() == at::kFloat, "thinkdiff_hip::flux_inpaint_mask: mask must be uint8 or float32, got ", mask.scalar_type());
  const int64_t H = mask.size(0), W = mask.size(1);
  TORCH_CHECK(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0 && C > 0, "thinkdiff_hip::flux_inpaint_mask: H, W must be positive multiples of 16, got ", mask.sizes());
  DeviceGuard guard(mask.device());
  at::Tensor out = at::empty({(H / 16) * (W / 16), 4 * C}, mask.options().dtype(at::kBFloat16));
  ok(td_flux_inpaint_mask(mask.data_ptr(), u8 ? TD_INPAINT_MASK_U8_HW : TD_INPAINT_MASK_F32_HW, (int)H, (int)W, (int)C, out.data_ptr(), stream_of(mask)));
  return out;
}

at::Tensor flux_pack_latents(const at::Tensor& latents) {            // [C,H,W] -> [(H/2)(W/2), 4C]
  check_rows(latents, "latents");
  TORCH_CHECK(latents.dim() == 3 && latents.is_contiguous(), "thinkdiff_hip::flux_pack_latents: contiguous [C,H,W]");
  const int64_t C = latents.size(0), H = latents.size(1), W = latents.size(2);
  DeviceGuard guard(latents.device());
  at::Tensor out = at::empty({(H / 2) * (W / 2), C * 4}, latents.options());
  ok(td_flux_pack_latents(latents.data_ptr(), out.data_ptr(), (int)C, (int)H, (int)W, 0, 1.0f, 0.0f, stream_of(latents)));
  return out;
}

at::Tensor flux_unpack_latents(const at::Tensor& packed, int64_t C, int64_t H, int64_t W, double div, double add) {   // bf16(bf16(x / div) + add)
  check_rows(packed, "packed");
  TORCH_CHECK(packed.is_contiguous() && packed.numel() == C * H * W, "thinkdiff_hip::flux_unpack_latents: contiguous [(H/2)(W/2), 4C]");
  DeviceGuard guard(packed.device());
  at::Tensor out = at::empty({C, H, W}, packed.options());
  ok(td_flux_pack_latents(packed.data_ptr(), out.data_ptr(), (int)C, (int)H, (int)W, 1, (float)div, (float)add, stream_of(packed)));
  return out;
}

at::Tensor cls_avgpool2(const at::Tensor& tokens) {                  // [1+G*G, C] -> [1+(G/2)^2, C]
  check_rows(tokens, "tokens");
  TORCH_CHECK(tokens.dim() == 2 && tokens.is_contiguous(), "thinkdiff_hip::cls_avgpool2: contiguous [1+G*G, C]");
  int64_t G = 0;
  while ((G + 1) * (G + 1) <= tokens.size(0) - 1) ++G;
  TORCH_CHECK(G * G == tokens.size(0) - 1, "thinkdiff_hip::cls_avgpool2: token count must be 1 + G*G");
  DeviceGuard guard(tokens.device());
  at::Tensor out = at::empty({1 + (G / 2) * (G / 2), tokens.size(1)}, tokens.options());
  ok(td_cls_avgpool2_bf16(tokens.data_ptr(), out.data_ptr(), (int)G, (int)tokens.size(1), stream_of(tokens)));
  return out;
}

// PIL's Image.resize on the device (td_resize_coeffs + td_image_resize_u8): img uint8 [H, W, C] contiguous -> uint8 [out_h, out_w, out_channels or C], the bytes
// Pillow gives for `resample` 1 (LANCZOS), 2 (BILINEAR) or 3 (BICUBIC); C -> out_channels is 3 -> 3, 1 -> 1, 1 -> 3 or 4 -> 3 (Pillow's convert("RGB")).  The
// coefficient tables are made on the host per call and uploaded on the current stream ahead of the launch, so no device copy is shared between streams.
at::Tensor image_resize_u8(const at::Tensor& img, int64_t out_h, int64_t out_w, int64_t resample, c10::optional<int64_t> out_channels) {
  TORCH_CHECK(img.is_cuda() && img.scalar_type() == at::kByte && img.dim() == 3 && img.is_contiguous(),
              "thinkdiff_hip::image_resize_u8: img must be a contiguous uint8 GPU tensor [H, W, C], got ", img.sizes(), " ", img.scalar_type());
  const int64_t in_h = img.size(0), in_w = img.size(1), in_c = img.size(2), out_c = out_channels.value_or(in_c);
  TORCH_CHECK(in_h > 0 && in_w > 0 && in_h < (1ll << 31) && in_w < (1ll << 31) && out_h > 0 && out_w > 0 && out_h < (1ll << 31) && out_w < (1ll << 31),
              "thinkdiff_hip::image_resize_u8: sizes ", in_h, "x", in_w, " -> ", out_h, "x", out_w, " must be 1 .. 2^31 - 1");
  TORCH_CHECK(in_c >= 1 && in_c <= 4 && out_c >= 1 && out_c <= 4, "thinkdiff_hip::image_resize_u8: channels ", in_c, " -> ", out_c, " are not built");
  const bool horiz = out_w != in_w, vert = out_h != in_h;
  int kh = 0, kv = 0;
  if (horiz) ok(td_resize_coeffs((int)in_w, (int)out_w, (int)resample, nullptr, nullptr, &kh));
  if (vert) ok(td_resize_coeffs((int)in_h, (int)out_h, (int)resample, nullptr, nullptr, &kv));
  // one host buffer [h_bounds | h_kk | v_bounds | v_kk], one upload
  const int64_t o_hk = horiz ? 2 * out_w : 0, o_vb = o_hk + (horiz ? out_w * kh : 0), o_vk = o_vb + (vert ? 2 * out_h : 0), total = o_vk + (vert ? out_h * kv : 0);
  DeviceGuard guard(img.device());
  at::Tensor tab_dev;
  const int32_t* t = nullptr;
  if (total > 0) {
    at::Tensor tab = at::empty({total}, at::TensorOptions().dtype(at::kInt));
    int32_t* h = tab.data_ptr<int32_t>();
    if (horiz) ok(td_resize_coeffs((int)in_w, (int)out_w, (int)resample, h, h + o_hk, &kh));
    if (vert) ok(td_resize_coeffs((int)in_h, (int)out_h, (int)resample, h + o_vb, h + o_vk, &kv));
    tab_dev = tab.to(img.device());
    t = tab_dev.data_ptr<int32_t>();
  }
  at::Tensor out = at::empty({out_h, out_w, out_c}, img.options());
  at::Tensor tmp;
  if (horiz && vert) tmp = at::empty({in_h, out_w, out_c}, img.options());
  ok(td_image_resize_u8(img.data_ptr(), (int)in_h, (int)in_w, (int)in_c, out.data_ptr(), (int)out_h, (int)out_w, (int)out_c, horiz ? t : nullptr, horiz ? t + o_hk : nullptr, kh,
                        vert ? t + o_vb : nullptr, vert ? t + o_vk : nullptr, kv, tmp.defined() ? tmp.data_ptr() : nullptr, stream_of(img)));
  return out;
}

// one token per row of bf16 logits: temperature / top-p, drawn from (seed, offset, row); temperature <= 0: greedy
at::Tensor sample_top_p(const at::Tensor& logits, double temperature, double top_p, int64_t seed, int64_t offset) {
  check_rows(logits, "logits");
  at::Tensor x = logits.dim() == 1 ? logits.unsqueeze(0) : logits;
  TORCH_CHECK(x.dim() == 2, "thinkdiff_hip::sample_top_p: logits [rows, vocab]");
  DeviceGuard guard(x.device());
  at::Tensor out = at::empty({x.size(0)}, x.options().dtype(at::kInt));
  ok(td_sample_top_p_bf16(x.data_ptr(), x.stride(0), (int)x.size(0), (int)x.size(1), (float)temperature, (float)top_p, (uint64_t)seed,
                          (uint64_t)offset, (int32_t*)out.data_ptr(), stream_of(x)));
  return out;
}

// one token per row, every row under its own TdSampleRow (params: uint8 [rows, sizeof(TdSampleRow)] on the device, offsets: int64 [rows]); state: a
// td_sampler handle as an int (thinkdiff._hip.Sampler.handle) or None when no row names a history slot
at::Tensor sample_rows(const at::Tensor& logits, const at::Tensor& params, const at::Tensor& offsets, c10::optional<int64_t> state, bool update_state) {
  check_rows(logits, "logits");
  at::Tensor x = logits.dim() == 1 ? logits.unsqueeze(0) : logits;
  TORCH_CHECK(x.dim() == 2, "thinkdiff_hip::sample_rows: logits [rows, vocab]");
  const int64_t rows = x.size(0);
  TORCH_CHECK(params.is_cuda() && params.device() == x.device() && params.scalar_type() == at::kByte && params.is_contiguous() &&
              params.numel() == rows * (int64_t)td_sample_row_size(),
              "thinkdiff_hip::sample_rows: params must be a contiguous uint8 tensor of ", rows, " x ", td_sample_row_size(), " bytes on the logits' device");
  TORCH_CHECK(offsets.is_cuda() && offsets.device() == x.device() && offsets.scalar_type() == at::kLong && offsets.is_contiguous() && offsets.numel() == rows,
              "thinkdiff_hip::sample_rows: offsets must be a contiguous int64 tensor of ", rows, " entries on the logits' device");
  DeviceGuard guard(x.device());
  at::Tensor out = at::empty({rows}, x.options().dtype(at::kInt));
  const td_sampler* s = state.has_value() && *state != 0 ? reinterpret_cast<const td_sampler*>(*state) : nullptr;
  ok(td_sample_rows_bf16(s, x.data_ptr(), x.stride(0), (int)rows, (int)x.size(1), (const TdSampleRow*)params.data_ptr(), (const int64_t*)offsets.data_ptr(),
                         update_state ? 1 : 0, (int32_t*)out.data_ptr(), stream_of(x)));
  return out;
}

// sample_rows with the logit edits of slot edit_slots[row] applied to each row (edits: a td_logit_edits handle as an int, thinkdiff._hip.LogitEdits.handle;
// edit_slots: int32 [rows] on the logits' device, -1 = none).  edits None: sample_rows.
at::Tensor sample_rows_edit(const at::Tensor& logits, const at::Tensor& params, const at::Tensor& offsets, c10::optional<int64_t> state, bool update_state,
                            c10::optional<int64_t> edits, const c10::optional<at::Tensor>& edit_slots) {
  const td_logit_edits* e = edits.has_value() && *edits != 0 ? reinterpret_cast<const td_logit_edits*>(*edits) : nullptr;
  if (!e) return sample_rows(logits, params, offsets, state, update_state);
  check_rows(logits, "logits");
  at::Tensor x = logits.dim() == 1 ? logits.unsqueeze(0) : logits;
  TORCH_CHECK(x.dim() == 2, "thinkdiff_hip::sample_rows_edit: logits [rows, vocab]");
  const int64_t rows = x.size(0);
  TORCH_CHECK(params.is_cuda() && params.device() == x.device() && params.scalar_type() == at::kByte && params.is_contiguous() &&
              params.numel() == rows * (int64_t)td_sample_row_size(),
              "thinkdiff_hip::sample_rows_edit: params must be a contiguous uint8 tensor of ", rows, " x ", td_sample_row_size(), " bytes on the logits' device");
  TORCH_CHECK(offsets.is_cuda() && offsets.device() == x.device() && offsets.scalar_type() == at::kLong && offsets.is_contiguous() && offsets.numel() == rows,
              "thinkdiff_hip::sample_rows_edit: offsets must be a contiguous int64 tensor of ", rows, " entries on the logits' device");
  TORCH_CHECK(edit_slots.has_value() && edit_slots->is_cuda() && edit_slots->device() == x.device() && edit_slots->scalar_type() == at::kInt &&
              edit_slots->is_contiguous() && edit_slots->numel() == rows,
              "thinkdiff_hip::sample_rows_edit: edit_slots must be a contiguous int32 tensor of ", rows, " entries on the logits' device");
  DeviceGuard guard(x.device());
  at::Tensor out = at::empty({rows}, x.options().dtype(at::kInt));
  const td_sampler* s = state.has_value() && *state != 0 ? reinterpret_cast<const td_sampler*>(*state) : nullptr;
  ok(td_sample_rows_edit_bf16(s, e, (const int32_t*)edit_slots->data_ptr(), x.data_ptr(), x.stride(0), (int)rows, (int)x.size(1),
                              (const TdSampleRow*)params.data_ptr(), (const int64_t*)offsets.data_ptr(), update_state ? 1 : 0, (int32_t*)out.data_ptr(),
                              stream_of(x)));
  return out;
}

// raw-logit logprobs per row: (lp_sampled fp32 [rows], rank int32 [rows], top_ids int32 [rows, top_cap], top_lp fp32 [rows, top_cap]); ids / n_top: int32
// [rows] on the logits' device.  Rows with n_top < 0 are skipped by the kernel: their outputs are pre-filled here (lp -inf, rank 0, ids -1).
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> logprobs_rows(const at::Tensor& logits, const at::Tensor& ids, const at::Tensor& n_top, int64_t top_cap) {
  check_rows(logits, "logits");
  at::Tensor x = logits.dim() == 1 ? logits.unsqueeze(0) : logits;
  TORCH_CHECK(x.dim() == 2, "thinkdiff_hip::logprobs_rows: logits [rows, vocab]");
  const int64_t rows = x.size(0);
  TORCH_CHECK(top_cap >= 0 && top_cap <= TD_MAX_LOGPROBS, "thinkdiff_hip::logprobs_rows: top_cap must be in 0..", TD_MAX_LOGPROBS, ", got ", top_cap);
  for (const at::Tensor* t : {&ids, &n_top})
    TORCH_CHECK(t->is_cuda() && t->device() == x.device() && t->scalar_type() == at::kInt && t->is_contiguous() && t->numel() == rows,
                "thinkdiff_hip::logprobs_rows: ids and n_top must be contiguous int32 tensors of ", rows, " entries on the logits' device");
  DeviceGuard guard(x.device());
  const auto inf = std::numeric_limits<float>::infinity();
  at::Tensor lp = at::full({rows}, -inf, x.options().dtype(at::kFloat));
  at::Tensor rank = at::zeros({rows}, x.options().dtype(at::kInt));
  at::Tensor top_ids = at::full({rows, top_cap}, -1, x.options().dtype(at::kInt));
  at::Tensor top_lp = at::full({rows, top_cap}, -inf, x.options().dtype(at::kFloat));
  ok(td_logprobs_rows_bf16(x.data_ptr(), x.stride(0), (int)rows, (int)x.size(1), (const int32_t*)ids.data_ptr(), (const int32_t*)n_top.data_ptr(), (int)top_cap,
                           (float*)lp.data_ptr(), (int32_t*)rank.data_ptr(), top_cap ? (int32_t*)top_ids.data_ptr() : nullptr,
                           top_cap ? (float*)top_lp.data_ptr() : nullptr, stream_of(x)));
  return std::make_tuple(lp, rank, top_ids, top_lp);
}

// ---- the engines: the denoise loop itself goes through the dispatcher ----------------------------------------------------------------
// An engine is a stateful C++ object behind the C ABI (weights, workspaces, prepared conditioning); the ops take its handle as an int (the
// td_flux* / td_vae* value, as thinkdiff.models.* hold it) and check every tensor against what the prepared context expects.
td_flux* flux_of(int64_t h) {
  TORCH_CHECK(h != 0, "thinkdiff_hip: null FLUX engine handle");
  return (td_flux*)(uintptr_t)h;
}
void check_latents(td_flux* f, const at::Tensor& x, const char* name) {
  int si = 0, c = 0, n = 0;
  ok(td_flux_prepared_shape(f, &si, nullptr, &c, &n));
  check_rows(x, name);
  TORCH_CHECK(si > 0 && n > 0, "thinkdiff_hip: the FLUX context has no condition / timesteps prepared");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && x.size(0) == si && x.size(1) == c, "thinkdiff_hip: ", name, " must be contiguous [", si, ", ", c, "] bf16, got ", x.sizes());
}
// the channel condition of a conditioned engine (FLUX.1 Fill / Canny / Depth): cond [S_img, in_channels - out_channels] bf16, copied beside
// the latents' columns of this context's x_embedder operand (td_flux_set_channel_condition)
void flux_set_channel_condition(int64_t engine, const at::Tensor& cond) {
  td_flux* f = flux_of(engine);
  int si = 0, cin = 0, cc = 0;
  ok(td_flux_prepared_shape(f, &si, nullptr, nullptr, nullptr));
  ok(td_flux_input_shape(f, &cin, &cc, nullptr));
  TORCH_CHECK(cc > 0, "thinkdiff_hip::flux_set_channel_condition: this engine takes no channel condition (x_embedder reads the ", cin, " latent channels only)");
  TORCH_CHECK(si > 0, "thinkdiff_hip::flux_set_channel_condition: the FLUX context has no condition prepared (set_condition fixes the token count)");
  check_rows(cond, "cond");
  TORCH_CHECK(cond.dim() == 2 && cond.is_contiguous() && cond.size(0) == si && cond.size(1) == cc,
              "thinkdiff_hip::flux_set_channel_condition: cond must be contiguous [", si, ", ", cc, "] bf16, got ", cond.sizes());
  DeviceGuard guard(cond.device());
  ok(td_flux_set_channel_condition(f, cond.data_ptr(), stream_of(cond)));
}
// FLUX.1 Kontext's reference tokens of one image: ref_latents [S_ref, out_channels] bf16, ref_ids [S_ref, 3] fp32; they join this context's
// image stream behind the latents in every forward (td_flux_set_reference_tokens).  S_ref == 0 clears.
void flux_set_reference_tokens(int64_t engine, const at::Tensor& ref_latents, const at::Tensor& ref_ids) {
  td_flux* f = flux_of(engine);
  int si = 0, c = 0;
  ok(td_flux_prepared_shape(f, &si, nullptr, &c, nullptr));
  TORCH_CHECK(si > 0, "thinkdiff_hip::flux_set_reference_tokens: the FLUX context has no condition prepared (set_condition fixes the token counts)");
  check_rows(ref_latents, "ref_latents"); check_rows(ref_ids, "ref_ids", at::kFloat); same_device(ref_ids, "ref_ids", ref_latents);
  TORCH_CHECK(ref_latents.dim() == 2 && ref_latents.is_contiguous() && ref_latents.size(1) == c,
              "thinkdiff_hip::flux_set_reference_tokens: ref_latents must be contiguous [S_ref, ", c, "] bf16, got ", ref_latents.sizes());
  const int64_t sr = ref_latents.size(0);
  TORCH_CHECK(ref_ids.dim() == 2 && ref_ids.is_contiguous() && ref_ids.size(0) == sr && ref_ids.size(1) == 3,
              "thinkdiff_hip::flux_set_reference_tokens: ref_ids must be contiguous [", sr, ", 3] fp32, got ", ref_ids.sizes());
  DeviceGuard guard(ref_latents.device());
  ok(td_flux_set_reference_tokens(f, sr ? ref_latents.data_ptr() : nullptr, (int)sr, sr ? (const float*)ref_ids.data_ptr() : nullptr, stream_of(ref_latents)));
}
// velocity = FluxTransformer2DModel.forward(latents) at prepared step `step`
at::Tensor& flux_forward_(int64_t engine, const at::Tensor& latents, int64_t step, at::Tensor& velocity) {
  td_flux* f = flux_of(engine);
  check_latents(f, latents, "latents"); check_latents(f, velocity, "velocity"); same_device(velocity, "velocity", latents);
  DeviceGuard guard(latents.device());
  ok(td_flux_forward(f, latents.data_ptr(), (int)step, velocity.data_ptr(), stream_of(latents)));
  return velocity;
}
// the whole Euler flow-matching loop in place: FluxPipeline.__call__'s denoising loop (transformer + scheduler.step per sigma)
at::Tensor& flux_denoise_(int64_t engine, at::Tensor& latents, at::ArrayRef<double> sigmas) {
  td_flux* f = flux_of(engine);
  check_latents(f, latents, "latents");
  TORCH_CHECK(sigmas.size() >= 2, "thinkdiff_hip::flux_denoise_: sigmas needs n + 1 >= 2 entries");
  std::vector<float> sg(sigmas.begin(), sigmas.end());
  DeviceGuard guard(latents.device());
  ok(td_flux_denoise(f, latents.data_ptr(), sg.data(), (int)sg.size() - 1, stream_of(latents)));
  return latents;
}
// FluxKontextPipeline's loop under true classifier-free guidance, in place: per step the transformer on both contexts, then flux_cfg_step_
at::Tensor& flux_denoise_cfg_(int64_t engine_pos, int64_t engine_neg, at::Tensor& latents, at::ArrayRef<double> sigmas, double scale) {
  td_flux* fp = flux_of(engine_pos);
  td_flux* fn = flux_of(engine_neg);
  check_latents(fp, latents, "latents (positive context)"); check_latents(fn, latents, "latents (negative context)");
  TORCH_CHECK(sigmas.size() >= 2, "thinkdiff_hip::flux_denoise_cfg_: sigmas needs n + 1 >= 2 entries");
  std::vector<float> sg(sigmas.begin(), sigmas.end());
  DeviceGuard guard(latents.device());
  ok(td_flux_denoise_cfg(fp, fn, latents.data_ptr(), sg.data(), (int)sg.size() - 1, (float)scale, stream_of(latents)));
  return latents;
}
// the same for several prepared contexts (a parent and its forks) at once, context k on streams[k] (hipStream_t values)
void flux_denoise_multi_(at::ArrayRef<int64_t> engines, at::TensorList latents, at::ArrayRef<double> sigmas, at::ArrayRef<int64_t> streams) {
  TORCH_CHECK(!engines.empty() && engines.size() == latents.size() && engines.size() == streams.size(), "thinkdiff_hip::flux_denoise_multi_: one latent tensor and one stream per engine");
  TORCH_CHECK(sigmas.size() >= 2, "thinkdiff_hip::flux_denoise_multi_: sigmas needs n + 1 >= 2 entries");
  std::vector<td_flux*> fs; std::vector<void*> ls, ss;
  for (size_t k = 0; k < engines.size(); ++k) {
    fs.push_back(flux_of(engines[k]));
    check_latents(fs.back(), latents[k], "latents[k]"); same_device(latents[k], "latents[k]", latents[0]);
    ls.push_back(latents[k].data_ptr()); ss.push_back((void*)(uintptr_t)streams[k]);
  }
  std::vector<float> sg(sigmas.begin(), sigmas.end());
  DeviceGuard guard(latents[0].device());
  ok(td_flux_denoise_multi(fs.data(), ls.data(), (int)fs.size(), sg.data(), (int)sg.size() - 1, ss.data()));
}
// FluxInpaintPipeline's loop in place: flux_denoise_ with the inpainting step (flux_inpaint_step_) after every forward; image_latents, noise
// and mask are [S_img, out_channels] like the latents and must not overlap them
at::Tensor& flux_denoise_inpaint_(int64_t engine, at::Tensor& latents, at::ArrayRef<double> sigmas, const at::Tensor& image_latents,
                                  const at::Tensor& noise, const at::Tensor& mask) {
  td_flux* f = flux_of(engine);
  check_latents(f, latents, "latents");
  check_latents(f, image_latents, "image_latents"); check_latents(f, noise, "noise"); check_latents(f, mask, "mask");
  same_device(image_latents, "image_latents", latents); same_device(noise, "noise", latents); same_device(mask, "mask", latents);
  TORCH_CHECK(sigmas.size() >= 2, "thinkdiff_hip::flux_denoise_inpaint_: sigmas needs n + 1 >= 2 entries");
  std::vector<float> sg(sigmas.begin(), sigmas.end());
  DeviceGuard guard(latents.device());
  ok(td_flux_denoise_inpaint(f, latents.data_ptr(), sg.data(), (int)sg.size() - 1, image_latents.data_ptr(), noise.data_ptr(), mask.data_ptr(),
                             stream_of(latents)));
  return latents;
}
// the same for several prepared contexts at once, context k on streams[k], blended with image_latents[k], noise[k], mask[k]
void flux_denoise_multi_inpaint_(at::ArrayRef<int64_t> engines, at::TensorList latents, at::ArrayRef<double> sigmas, at::TensorList image_latents,
                                 at::TensorList noise, at::TensorList mask, at::ArrayRef<int64_t> streams) {
  const size_t n = engines.size();
  TORCH_CHECK(n > 0 && latents.size() == n && streams.size() == n && image_latents.size() == n && noise.size() == n && mask.size() == n,
              "thinkdiff_hip::flux_denoise_multi_inpaint_: one latent tensor, blend triple and stream per engine");
  TORCH_CHECK(sigmas.size() >= 2, "thinkdiff_hip::flux_denoise_multi_inpaint_: sigmas needs n + 1 >= 2 entries");
  std::vector<td_flux*> fs; std::vector<void*> ls, ss; std::vector<const void*> zs, ns, ms;
  for (size_t k = 0; k < n; ++k) {
    fs.push_back(flux_of(engines[k]));
    check_latents(fs.back(), latents[k], "latents[k]"); same_device(latents[k], "latents[k]", latents[0]);
    check_latents(fs.back(), image_latents[k], "image_latents[k]"); same_device(image_latents[k], "image_latents[k]", latents[0]);
    check_latents(fs.back(), noise[k], "noise[k]"); same_device(noise[k], "noise[k]", latents[0]);
    check_latents(fs.back(), mask[k], "mask[k]"); same_device(mask[k], "mask[k]", latents[0]);
    ls.push_back(latents[k].data_ptr()); ss.push_back((void*)(uintptr_t)streams[k]);
    zs.push_back(image_latents[k].data_ptr()); ns.push_back(noise[k].data_ptr()); ms.push_back(mask[k].data_ptr());
  }
  std::vector<float> sg(sigmas.begin(), sigmas.end());
  DeviceGuard guard(latents[0].device());
  ok(td_flux_denoise_multi_inpaint(fs.data(), ls.data(), (int)n, sg.data(), (int)sg.size() - 1, zs.data(), ns.data(), ms.data(), ss.data()));
}
// AutoencoderKL.decode + VaeImageProcessor.postprocess: packed latents [(h/2)(w/2), 4C] -> uint8 [H, W, 3] (8h x 8w for the FLUX.1 VAE)
at::Tensor vae_decode_u8(int64_t engine, const at::Tensor& packed, int64_t h, int64_t w, double scaling_factor, double shift_factor) {
  TORCH_CHECK(engine != 0, "thinkdiff_hip: null VAE engine handle");
  check_rows(packed, "packed");
  int H = 0, W = 0, pc = 0;
  TORCH_CHECK(h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0, "thinkdiff_hip::vae_decode_u8: even latent height and width");
  ok(td_vae_output_shape((const td_vae*)(uintptr_t)engine, (int)h, (int)w, &H, &W, &pc));
  TORCH_CHECK(packed.dim() == 2 && packed.is_contiguous() && packed.size(0) == (h / 2) * (w / 2) && packed.size(1) == pc,
              "thinkdiff_hip::vae_decode_u8: packed must be contiguous [(h/2)(w/2) = ", (h / 2) * (w / 2), ", ", pc, "] bf16, got ", packed.sizes());
  DeviceGuard guard(packed.device());
  at::Tensor img = at::empty({H, W, 3}, packed.options().dtype(at::kByte));
  ok(td_vae_decode((td_vae*)(uintptr_t)engine, packed.data_ptr(), (int)h, (int)w, (float)scaling_factor, (float)shift_factor, img.data_ptr(), nullptr, stream_of(packed)));
  return img;
}
// VaeImageProcessor.preprocess + AutoencoderKL.encode up to the posterior's parameters: image uint8 [H, W, 3] or float32 [3, H, W] in [0, 1]
// -> moments [(H/8)(W/8), 2 x latent_channels] bf16 (mean | logvar, NHWC) on a td_vae_enc* engine
at::Tensor vae_encode_moments(int64_t engine, const at::Tensor& image, int64_t H, int64_t W) {
  TORCH_CHECK(engine != 0, "thinkdiff_hip: null VAE encoder handle");
  TORCH_CHECK(image.is_cuda() && image.is_contiguous(), "thinkdiff_hip::vae_encode_moments: image must be a contiguous GPU tensor");
  const bool u8 = image.scalar_type() == at::kByte;
  TORCH_CHECK(u8 || image.scalar_type() == at::kFloat, "thinkdiff_hip::vae_encode_moments: image must be uint8 [H, W, 3] or float32 [3, H, W], got ", image.scalar_type());
  TORCH_CHECK(u8 ? image.sizes() == at::IntArrayRef({H, W, 3}) : image.sizes() == at::IntArrayRef({3, H, W}),
              "thinkdiff_hip::vae_encode_moments: image must be ", u8 ? "uint8 [H, W, 3]" : "float32 [3, H, W]", " with H = ", H, ", W = ", W, ", got ", image.sizes());
  int h = 0, w = 0, mc = 0;
  ok(td_vae_enc_output_shape((const td_vae_enc*)(uintptr_t)engine, (int)H, (int)W, &h, &w, &mc));
  DeviceGuard guard(image.device());
  at::Tensor mom = at::empty({(int64_t)h * w, mc}, image.options().dtype(at::kBFloat16));
  ok(td_vae_encode((td_vae_enc*)(uintptr_t)engine, image.data_ptr(), u8 ? TD_IMAGE_U8_HWC : TD_IMAGE_F32_CHW, (int)H, (int)W, mom.data_ptr(), stream_of(image)));
  return mom;
}
// a [H, W] mask for the FLUX.1 Fill kernels: uint8 or float32, contiguous, on `like`'s device; returns its TD_INPAINT_MASK_* format
int fill_mask_format(const at::Tensor& mask, const at::Tensor& like, int64_t H, int64_t W, const char* op) {
  TORCH_CHECK(mask.is_cuda() && mask.is_contiguous() && mask.dim() == 2 && mask.size(0) == H && mask.size(1) == W,
              "thinkdiff_hip::", op, ": mask must be a contiguous GPU tensor [H = ", H, ", W = ", W, "], got ", mask.sizes());
  same_device(mask, "mask", like);
  const bool u8 = mask.scalar_type() == at::kByte;
  TORCH_CHECK(u8 || mask.scalar_type() == at::kFloat, "thinkdiff_hip::", op, ": mask must be uint8 or float32, got ", mask.scalar_type());
  return u8 ? TD_INPAINT_MASK_U8_HW : TD_INPAINT_MASK_F32_HW;
}
// vae_encode_moments of image * (1 - binarize(mask)) (FLUX.1 Fill's masked image): mask uint8 or float32 [H, W] at full resolution
at::Tensor vae_encode_moments_masked(int64_t engine, const at::Tensor& image, const at::Tensor& mask, int64_t H, int64_t W) {
  TORCH_CHECK(engine != 0, "thinkdiff_hip: null VAE encoder handle");
  TORCH_CHECK(image.is_cuda() && image.is_contiguous(), "thinkdiff_hip::vae_encode_moments_masked: image must be a contiguous GPU tensor");
  const bool u8 = image.scalar_type() == at::kByte;
  TORCH_CHECK(u8 || image.scalar_type() == at::kFloat, "thinkdiff_hip::vae_encode_moments_masked: image must be uint8 [H, W, 3] or float32 [3, H, W], got ", image.scalar_type());
  TORCH_CHECK(u8 ? image.sizes() == at::IntArrayRef({H, W, 3}) : image.sizes() == at::IntArrayRef({3, H, W}),
              "thinkdiff_hip::vae_encode_moments_masked: image must be ", u8 ? "uint8 [H, W, 3]" : "float32 [3, H, W]", " with H = ", H, ", W = ", W, ", got ", image.sizes());
  const int mfmt = fill_mask_format(mask, image, H, W, "vae_encode_moments_masked");
  int h = 0, w = 0, mc = 0;
  ok(td_vae_enc_output_shape((const td_vae_enc*)(uintptr_t)engine, (int)H, (int)W, &h, &w, &mc));
  DeviceGuard guard(image.device());
  at::Tensor mom = at::empty({(int64_t)h * w, mc}, image.options().dtype(at::kBFloat16));
  ok(td_vae_encode_masked((td_vae_enc*)(uintptr_t)engine, image.data_ptr(), u8 ? TD_IMAGE_U8_HWC : TD_IMAGE_F32_CHW, mask.data_ptr(), mfmt, (int)H, (int)W,
                          mom.data_ptr(), stream_of(image)));
  return mom;
}
// FLUX.1 Fill's channel condition of one image: packed (sample(moments, eps) - shift) * scaling | the unshuffled binarized mask ->
// [(H/16)(W/16), 4C + 256] bf16 (td_flux_fill_condition); moments [(H/8)(W/8), 2C] of the masked image
at::Tensor flux_fill_condition(const at::Tensor& moments, const c10::optional<at::Tensor>& eps, const at::Tensor& mask, double scaling_factor,
                               double shift_factor, int64_t H, int64_t W) {
  check_rows(moments, "moments");
  TORCH_CHECK(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "thinkdiff_hip::flux_fill_condition: H, W must be positive multiples of 16, got ", H, " x ", W);
  const int64_t h = H / 8, w = W / 8;
  TORCH_CHECK(moments.dim() == 2 && moments.is_contiguous() && moments.size(0) == h * w && moments.size(1) % 4 == 0 && moments.size(1) > 0,
              "thinkdiff_hip::flux_fill_condition: moments must be contiguous [(H/8)(W/8) = ", h * w, ", 2C] bf16 with C even, got ", moments.sizes());
  const int64_t C = moments.size(1) / 2;
  check_vec(eps, "eps", moments, C * h * w);
  const int mfmt = fill_mask_format(mask, moments, H, W, "flux_fill_condition");
  DeviceGuard guard(moments.device());
  at::Tensor out = at::empty({(h / 2) * (w / 2), 4 * C + 256}, moments.options());
  ok(td_flux_fill_condition(moments.data_ptr(), P(eps), mask.data_ptr(), mfmt, (int)H, (int)W, (float)scaling_factor, (float)shift_factor, (int)C,
                            out.data_ptr(), stream_of(moments)));
  return out;
}
// posterior sample / mode + shift / scale + scale_noise + _pack_latents: moments [h*w, 2C] -> packed latents [(h/2)(w/2), 4C]
at::Tensor vae_latents_from_moments(const at::Tensor& moments, const c10::optional<at::Tensor>& eps, const c10::optional<at::Tensor>& noise, double sigma,
                                    double scaling_factor, double shift_factor, int64_t h, int64_t w) {
  check_rows(moments, "moments");
  TORCH_CHECK(h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0, "thinkdiff_hip::vae_latents_from_moments: even latent height and width");
  TORCH_CHECK(moments.dim() == 2 && moments.is_contiguous() && moments.size(0) == h * w && moments.size(1) % 2 == 0,
              "thinkdiff_hip::vae_latents_from_moments: moments must be contiguous [h*w = ", h * w, ", 2C] bf16, got ", moments.sizes());
  const int64_t C = moments.size(1) / 2;
  check_vec(eps, "eps", moments, C * h * w);
  check_vec(noise, "noise", moments, C * h * w);
  DeviceGuard guard(moments.device());
  at::Tensor out = at::empty({(h / 2) * (w / 2), 4 * C}, moments.options());
  ok(td_vae_latents_from_moments(moments.data_ptr(), P(eps), P(noise), (float)sigma, (float)scaling_factor, (float)shift_factor, (int)C, (int)h, (int)w,
                                 out.data_ptr(), stream_of(moments)));
  return out;
}
// the joint attention with QK^T and P.V on the e4m3 MFMA (td_attention_fp8): q, k, v [S, >= H*128] bf16 views
at::Tensor attention_fp8(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, int64_t H, double scale) {
  check_rows(q, "q"); check_rows(k, "k"); check_rows(v, "v"); same_device(k, "k", q); same_device(v, "v", q);
  TORCH_CHECK(q.dim() == 2 && k.dim() == 2 && v.dim() == 2 && H > 0 && q.size(1) >= H * 128 && k.size(1) >= H * 128 && v.size(1) >= H * 128 && k.size(0) == v.size(0) &&
              k.stride(0) == v.stride(0), "thinkdiff_hip::attention_fp8: q [Sq, >= H*128], k / v [Skv, >= H*128] with equal row strides");
  DeviceGuard guard(q.device());
  at::Tensor out = at::empty({q.size(0), H * 128}, q.options());
  at::Tensor ws = at::empty({(int64_t)td_attention_fp8_workspace_bytes((int)q.size(0), (int)k.size(0), (int)H)}, q.options().dtype(at::kByte));
  ok(td_attention_fp8(q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0), out.data_ptr(), out.stride(0), (int)q.size(0), (int)k.size(0), (int)H,
                      (float)scale, ws.data_ptr(), stream_of(q)));
  return out;
}

// ---- LoRA adapters --------------------------------------------------------------------------------------------------------------------------
// peft's `weight + scaling * (lora_B.weight @ lora_A.weight)` for several pairs at once, one rounding (td_lora_merge_bf16): w [N, K], A[i] [r_i, K],
// B[i] [N, r_i] bf16 contiguous -> a new [N, K] tensor.  The kernel's operand form of every pair is made here, per call (the engine makes it once).
at::Tensor lora_merge(const at::Tensor& w, at::TensorList A, at::TensorList B, at::ArrayRef<double> scales) {
  check_rows(w, "w");
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous(), "thinkdiff_hip::lora_merge: w must be contiguous [N, K]");
  TORCH_CHECK(A.size() == B.size() && A.size() == scales.size(), "thinkdiff_hip::lora_merge: ", A.size(), " A, ", B.size(), " B, ", scales.size(), " scales");
  TORCH_CHECK(A.size() <= TD_LORA_MAX_ADAPTERS, "thinkdiff_hip::lora_merge: ", A.size(), " adapters, one call takes at most ", TD_LORA_MAX_ADAPTERS);
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(N < (1ll << 31) && K < (1ll << 31), "thinkdiff_hip::lora_merge: w is too large");
  DeviceGuard guard(w.device());
  std::vector<at::Tensor> packed;
  std::vector<const void*> ptrs;
  std::vector<int> ranks;
  std::vector<float> sc;
  for (size_t i = 0; i < A.size(); ++i) {
    TORCH_CHECK(A[i].dim() == 2 && B[i].dim() == 2 && A[i].size(0) >= 1, "thinkdiff_hip::lora_merge: pair ", i, ": A [r, K], B [N, r] with r >= 1");
    const int64_t r = A[i].size(0);
    TORCH_CHECK(A[i].size(1) == K && B[i].size(0) == N && B[i].size(1) == r, "thinkdiff_hip::lora_merge: pair ", i, ": A ", A[i].sizes(), " / B ", B[i].sizes(),
                " do not fit w ", w.sizes());
    check_vec(A[i], "A", w, r * K); check_vec(B[i], "B", w, N * r);
    const size_t bytes = td_lora_packed_bytes((int)r, (int)N, (int)K);
    packed.push_back(at::empty({(int64_t)bytes}, w.options().dtype(at::kByte)));
    ok(td_lora_pack_bf16(A[i].data_ptr(), B[i].data_ptr(), (int)r, (int)N, (int)K, packed.back().data_ptr(), stream_of(w)));
    ptrs.push_back(packed.back().data_ptr()); ranks.push_back((int)r); sc.push_back((float)scales[i]);
  }
  at::Tensor out = at::empty_like(w);
  ok(td_lora_merge_bf16(w.data_ptr(), out.data_ptr(), (int)N, (int)K, (int)ptrs.size(), ptrs.data(), ranks.data(), sc.data(), stream_of(w)));
  return out;
}
// the same, into w itself (td_lora_merge_bf16 with w_out == w_base)
at::Tensor& lora_merge_(at::Tensor& w, at::TensorList A, at::TensorList B, at::ArrayRef<double> scales) {
  check_rows(w, "w");
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous(), "thinkdiff_hip::lora_merge_: w must be contiguous [N, K]");
  TORCH_CHECK(A.size() == B.size() && A.size() == scales.size(), "thinkdiff_hip::lora_merge_: ", A.size(), " A, ", B.size(), " B, ", scales.size(), " scales");
  TORCH_CHECK(A.size() <= TD_LORA_MAX_ADAPTERS, "thinkdiff_hip::lora_merge_: ", A.size(), " adapters, one call takes at most ", TD_LORA_MAX_ADAPTERS);
  const int64_t N = w.size(0), K = w.size(1);
  TORCH_CHECK(N < (1ll << 31) && K < (1ll << 31), "thinkdiff_hip::lora_merge_: w is too large");
  DeviceGuard guard(w.device());
  std::vector<at::Tensor> packed;
  std::vector<const void*> ptrs;
  std::vector<int> ranks;
  std::vector<float> sc;
  for (size_t i = 0; i < A.size(); ++i) {
    TORCH_CHECK(A[i].dim() == 2 && B[i].dim() == 2 && A[i].size(0) >= 1, "thinkdiff_hip::lora_merge_: pair ", i, ": A [r, K], B [N, r] with r >= 1");
    const int64_t r = A[i].size(0);
    TORCH_CHECK(A[i].size(1) == K && B[i].size(0) == N && B[i].size(1) == r, "thinkdiff_hip::lora_merge_: pair ", i, ": A ", A[i].sizes(), " / B ", B[i].sizes(),
                " do not fit w ", w.sizes());
    check_vec(A[i], "A", w, r * K); check_vec(B[i], "B", w, N * r);
    packed.push_back(at::empty({(int64_t)td_lora_packed_bytes((int)r, (int)N, (int)K)}, w.options().dtype(at::kByte)));
    ok(td_lora_pack_bf16(A[i].data_ptr(), B[i].data_ptr(), (int)r, (int)N, (int)K, packed.back().data_ptr(), stream_of(w)));
    ptrs.push_back(packed.back().data_ptr()); ranks.push_back((int)r); sc.push_back((float)scales[i]);
  }
  ok(td_lora_merge_bf16(w.data_ptr(), w.data_ptr(), (int)N, (int)K, (int)ptrs.size(), ptrs.data(), ranks.data(), sc.data(), stream_of(w)));
  return w;
}
// the row-indexed low-rank add (td_lora_rows_bf16; csrc/lora_rows.hip), in place on the output segments ys: ys[s][row] += scales[a] * B (bf16(A x[row])) for
// a = row_adapter[row] >= 0, one rounding.  A / B hold the pairs that exist, pair[a * len(ys) + s] the index of adapter a's pair for segment s in them or -1
// (the adapter does not touch the segment).  The kernels' operand form of every pair is made here, per call (the engine makes it once).
void lora_rows_(const at::Tensor& x, const at::Tensor& row_adapter, at::TensorList A, at::TensorList B, at::IntArrayRef pair, at::ArrayRef<double> scales,
                at::TensorList ys) {
  check_rows(x, "x");
  TORCH_CHECK(x.dim() == 2, "thinkdiff_hip::lora_rows_: x must be [rows, K]");
  const int64_t rows = x.size(0), K = x.size(1);
  const size_t n_ad = scales.size(), n_segs = ys.size();
  TORCH_CHECK(n_ad <= TD_LORA_MAX_ADAPTERS, "thinkdiff_hip::lora_rows_: ", n_ad, " adapters, one call takes at most ", TD_LORA_MAX_ADAPTERS);
  TORCH_CHECK(n_segs >= 1 && n_segs <= TD_LORA_ROWS_MAX_SEGS, "thinkdiff_hip::lora_rows_: ", n_segs, " output segments outside 1..", TD_LORA_ROWS_MAX_SEGS);
  TORCH_CHECK(A.size() == B.size() && pair.size() == n_ad * n_segs, "thinkdiff_hip::lora_rows_: ", A.size(), " A, ", B.size(), " B, ", pair.size(), " pair entries for ", n_ad,
              " adapters x ", n_segs, " segments");
  check_vec(row_adapter, "row_adapter", x, rows, at::kInt);
  TORCH_CHECK(rows >= 1 && rows < (1ll << 24) && K < (1ll << 31), "thinkdiff_hip::lora_rows_: x is empty or too large");
  std::vector<void*> yp; std::vector<int64_t> ld; std::vector<int> wd;
  for (size_t s = 0; s < n_segs; ++s) {
    check_rows(ys[s], "ys");
    TORCH_CHECK(ys[s].dim() == 2 && ys[s].size(0) == rows && ys[s].device() == x.device() && ys[s].size(1) < (1ll << 31), "thinkdiff_hip::lora_rows_: segment ", s, " must be [", rows,
                ", width] on ", x.device());
    yp.push_back(ys[s].data_ptr()); ld.push_back(ys[s].stride(0)); wd.push_back((int)ys[s].size(1));
  }
  DeviceGuard guard(x.device());
  std::vector<at::Tensor> packed(A.size());
  std::vector<const void*> ptrs(std::max<size_t>(1, n_ad * n_segs), nullptr);
  std::vector<int> ranks(std::max<size_t>(1, n_ad), 1);
  std::vector<float> sc(std::max<size_t>(1, n_ad), 0.f);
  int max_rank = 1;
  for (size_t a = 0; a < n_ad; ++a) {
    sc[a] = (float)scales[a];
    for (size_t s = 0; s < n_segs; ++s) {
      const int64_t i = pair[a * n_segs + s];
      if (i < 0) continue;
      TORCH_CHECK((size_t)i < A.size(), "thinkdiff_hip::lora_rows_: pair index ", i, " outside the ", A.size(), " pairs given");
      const int64_t N = wd[s];
      TORCH_CHECK(A[i].dim() == 2 && B[i].dim() == 2 && A[i].size(0) >= 1 && A[i].size(0) <= TD_LORA_ROWS_MAX_RANK, "thinkdiff_hip::lora_rows_: pair ", i,
                  ": A [r, K], B [N, r] with r in 1..", TD_LORA_ROWS_MAX_RANK);
      const int64_t r = A[i].size(0);
      TORCH_CHECK(A[i].size(1) == K && B[i].size(0) == N && B[i].size(1) == r, "thinkdiff_hip::lora_rows_: pair ", i, ": A ", A[i].sizes(), " / B ", B[i].sizes(),
                  " do not fit x ", x.sizes(), " and a segment of width ", N);
      check_vec(A[i], "A", x, r * K); check_vec(B[i], "B", x, N * r);
      if (!packed[i].defined()) {
        packed[i] = at::empty({(int64_t)td_lora_rows_packed_bytes((int)r, (int)N, (int)K)}, x.options().dtype(at::kByte));
        ok(td_lora_rows_pack_bf16(A[i].data_ptr(), B[i].data_ptr(), (int)r, (int)N, (int)K, packed[i].data_ptr(), stream_of(x)));
      }
      ptrs[a * n_segs + s] = packed[i].data_ptr();
      ranks[a] = (int)r;
      max_rank = std::max(max_rank, (int)r);
    }
  }
  const size_t wsb = td_lora_rows_workspace_bytes((int)rows, (int)K, (int)n_segs, max_rank);
  at::Tensor ws = at::empty({(int64_t)std::max<size_t>(16, wsb)}, x.options().dtype(at::kByte));
  ok(td_lora_rows_bf16(x.data_ptr(), x.stride(0), (int)rows, (int)K, (const int32_t*)row_adapter.data_ptr(), (int)n_ad, ptrs.data(), ranks.data(), sc.data(), (int)n_segs,
                       yp.data(), ld.data(), wd.data(), ws.data_ptr(), (size_t)ws.numel(), stream_of(x)));
}
// attach one pair to a Linear of the engine (td_flux_lora_load): A [r, K], B [N, r] against the [N, K] td_flux_param_shape reports
void flux_lora_load(int64_t engine, std::string adapter, std::string param, const at::Tensor& A, const at::Tensor& B, double scale) {
  TORCH_CHECK(engine != 0, "thinkdiff_hip: null engine handle");
  td_flux* f = (td_flux*)(uintptr_t)engine;
  int64_t N = 0, K = 0;
  ok(td_flux_param_shape(f, param.c_str(), &N, &K));
  check_rows(A, "A"); check_rows(B, "B"); same_device(B, "B", A);
  TORCH_CHECK(K > 1, "thinkdiff_hip::flux_lora_load: '", param, "' is not the weight of a Linear (", N, " elements, 1-D): bias and norm-scale deltas are not built");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(0) >= 1 && A.size(1) == K && B.size(0) == N && B.size(1) == A.size(0),
              "thinkdiff_hip::flux_lora_load: '", param, "' is [", N, ", ", K, "]: lora_A must be [r, ", K, "] and lora_B [", N, ", r], got ", A.sizes(), " / ", B.sizes());
  check_vec(A, "A", A, A.size(0) * K); check_vec(B, "B", A, N * A.size(0));
  DeviceGuard guard(A.device());
  ok(td_flux_lora_load(f, adapter.c_str(), param.c_str(), A.data_ptr(), B.data_ptr(), (int)A.size(0), (float)scale, stream_of(A)));
}
// The three ops below carry no tensor argument for the dispatcher to pick a backend from, so they are registered for every backend; they touch only
// the engine (device memory it owns, on the current HIP device and stream) and compute nothing themselves.
void* current_stream() { return (void*)c10::hip::getCurrentHIPStream().stream(); }
at::Tensor flux_read_param(int64_t engine, std::string name) {
  TORCH_CHECK(engine != 0, "thinkdiff_hip: null engine handle");
  td_flux* f = (td_flux*)(uintptr_t)engine;
  int64_t rows = 0, cols = 0;
  ok(td_flux_param_shape(f, name.c_str(), &rows, &cols));
  at::Tensor out = cols > 1 ? at::empty({rows, cols}, at::TensorOptions().dtype(at::kBFloat16).device(at::kCUDA))
                            : at::empty({rows}, at::TensorOptions().dtype(at::kBFloat16).device(at::kCUDA));
  ok(td_flux_read_param(f, name.c_str(), out.data_ptr(), out.numel(), current_stream()));
  return out;
}
// tests: a context's image-prompt tokens (block < 0) or double block `block`'s K (which 0) / V (1) of an IP-Adapter slot, as a new tensor
at::Tensor flux_ip_read(int64_t engine, int64_t slot, int64_t block, int64_t which) {
  TORCH_CHECK(engine != 0, "thinkdiff_hip: null engine handle");
  td_flux* f = (td_flux*)(uintptr_t)engine;
  int set = 0, n_keys = 0, D = 0, J = 0;
  ok(td_flux_ip_adapter_info(f, (int)slot, nullptr, nullptr, nullptr, &set, &n_keys));
  ok(td_flux_ip_widths(f, &J, &D));
  at::Tensor out = at::empty({n_keys, block < 0 ? J : D}, at::TensorOptions().dtype(at::kBFloat16).device(at::kCUDA));
  ok(td_flux_ip_read(f, (int)slot, (int)block, (int)which, out.data_ptr(), current_stream()));
  return out;
}
void flux_lora_set_adapters(int64_t engine, std::vector<std::string> names, at::ArrayRef<double> weights) {
  TORCH_CHECK(engine != 0, "thinkdiff_hip: null engine handle");
  TORCH_CHECK(names.size() == weights.size(), "thinkdiff_hip::flux_lora_set_adapters: ", names.size(), " names, ", weights.size(), " weights");
  std::vector<const char*> np;
  std::vector<float> wf;
  for (size_t i = 0; i < names.size(); ++i) { np.push_back(names[i].c_str()); wf.push_back((float)weights[i]); }
  ok(td_flux_lora_set_adapters((td_flux*)(uintptr_t)engine, np.data(), wf.data(), (int)np.size(), current_stream()));
}
void flux_lora_delete(int64_t engine, std::string adapter) {
  TORCH_CHECK(engine != 0, "thinkdiff_hip: null engine handle");
  if (adapter.empty()) ok(td_flux_lora_clear((td_flux*)(uintptr_t)engine, current_stream()));
  else ok(td_flux_lora_delete((td_flux*)(uintptr_t)engine, adapter.c_str(), current_stream()));
}

// KV fork on one plane (td_kv_fork_rows): plane [slots * slot_rows, row] of any dtype, rows [0, n_rows) of slot src_slot -> the same rows of every dst slot, in place
void kv_fork_rows(at::Tensor plane, int64_t slot_rows, int64_t src_slot, at::IntArrayRef dst_slots, int64_t n_rows) {
  TORCH_CHECK(plane.is_cuda(), "thinkdiff_hip: plane must live on the GPU");
  TORCH_CHECK(plane.dim() == 2 && plane.is_contiguous(), "thinkdiff_hip::kv_fork_rows: plane [slots * slot_rows, row] contiguous");
  TORCH_CHECK(slot_rows >= 1 && plane.size(0) % slot_rows == 0, "thinkdiff_hip::kv_fork_rows: slot_rows=", slot_rows, " does not divide the plane's ", plane.size(0), " rows");
  const int64_t slots = plane.size(0) / slot_rows;
  TORCH_CHECK(src_slot >= 0 && src_slot < slots, "thinkdiff_hip::kv_fork_rows: src_slot=", src_slot, " outside the plane's ", slots, " slots");
  std::vector<int> dst;
  for (int64_t d : dst_slots) {
    TORCH_CHECK(d >= 0 && d < slots, "thinkdiff_hip::kv_fork_rows: destination slot ", d, " outside the plane's ", slots, " slots");
    dst.push_back((int)d);
  }
  TORCH_CHECK(n_rows >= 0 && n_rows <= slot_rows, "thinkdiff_hip::kv_fork_rows: n_rows=", n_rows, " outside [0, slot_rows=", slot_rows, "]");
  DeviceGuard guard(plane.device());
  const TdKvPlane pl = {plane.data_ptr(), plane.size(1) * (int64_t)plane.element_size(), slot_rows};
  ok(td_kv_fork_rows(&pl, 1, (int)src_slot, dst.data(), (int)dst.size(), (int)n_rows, stream_of(plane)));
}

// KV gather on one plane (td_kv_gather_rows): row j with copy_src[j] >= 0 takes rows [0, n_rows[j]) of slot slots[copy_src[j]] into slot slots[j], in place;
// copy_src: int32 [len(slots)] on the plane's device, read by the kernel.  The caller vouches that no destination slot is a source of the same call.
void kv_gather_rows(at::Tensor plane, int64_t slot_rows, at::IntArrayRef slots, const at::Tensor& copy_src, at::IntArrayRef n_rows) {
  TORCH_CHECK(plane.is_cuda(), "thinkdiff_hip: plane must live on the GPU");
  TORCH_CHECK(plane.dim() == 2 && plane.is_contiguous(), "thinkdiff_hip::kv_gather_rows: plane [slots * slot_rows, row] contiguous");
  TORCH_CHECK(slot_rows >= 1 && plane.size(0) % slot_rows == 0, "thinkdiff_hip::kv_gather_rows: slot_rows=", slot_rows, " does not divide the plane's ", plane.size(0), " rows");
  const int64_t n_slots = plane.size(0) / slot_rows, n = (int64_t)slots.size();
  TORCH_CHECK(n >= 1 && n <= 256 && (int64_t)n_rows.size() == n, "thinkdiff_hip::kv_gather_rows: ", n, " slots (1..256) with ", n_rows.size(), " n_rows");
  TORCH_CHECK(copy_src.is_cuda() && copy_src.device() == plane.device() && copy_src.scalar_type() == at::kInt && copy_src.is_contiguous() && copy_src.numel() == n,
              "thinkdiff_hip::kv_gather_rows: copy_src must be a contiguous int32 tensor of ", n, " entries on the plane's device");
  std::vector<int> sl, nr;
  for (int64_t v : slots) {
    TORCH_CHECK(v >= 0 && v < n_slots, "thinkdiff_hip::kv_gather_rows: slot ", v, " outside the plane's ", n_slots, " slots");
    sl.push_back((int)v);
  }
  for (int64_t v : n_rows) {
    TORCH_CHECK(v >= 0 && v <= slot_rows, "thinkdiff_hip::kv_gather_rows: n_rows=", v, " outside [0, slot_rows=", slot_rows, "]");
    nr.push_back((int)v);
  }
  DeviceGuard guard(plane.device());
  const TdKvPlane pl = {plane.data_ptr(), plane.size(1) * (int64_t)plane.element_size(), slot_rows};
  ok(td_kv_gather_rows(&pl, 1, (int)n, sl.data(), (const int32_t*)copy_src.data_ptr(), nr.data(), stream_of(plane)));
}

// the beam-search step's choice and placement (td_beam_select): top_ids int32 / top_lp fp32 [R*W, cap] (logprobs_rows with n_top = 2W), cum_in fp32 and
// rank_in int32 [R*W]; the seven outputs are [R*W] tensors (slices of the caller's [T, R*W] logs) written in place
void beam_select(const at::Tensor& top_ids, const at::Tensor& top_lp, const at::Tensor& cum_in, const at::Tensor& rank_in, int64_t W, int64_t n_in, int64_t eos,
                 at::Tensor token, at::Tensor cum_out, at::Tensor rank_out, at::Tensor copy_src, at::Tensor parent, at::Tensor fin_flag, at::Tensor fin_cum) {
  TORCH_CHECK(top_ids.is_cuda(), "thinkdiff_hip: top_ids must live on the GPU");
  TORCH_CHECK(W >= 1 && W <= TD_MAX_BEAM_WIDTH, "thinkdiff_hip::beam_select: W=", W, " outside 1..", TD_MAX_BEAM_WIDTH);
  TORCH_CHECK(top_ids.dim() == 2 && top_ids.is_contiguous() && top_ids.scalar_type() == at::kInt && top_ids.size(0) >= 1 && top_ids.size(0) % W == 0,
              "thinkdiff_hip::beam_select: top_ids must be a contiguous int32 [R*W, cap] tensor");
  const int64_t rows = top_ids.size(0), cap = top_ids.size(1);
  TORCH_CHECK(top_lp.device() == top_ids.device() && top_lp.scalar_type() == at::kFloat && top_lp.is_contiguous() && top_lp.sizes() == top_ids.sizes(),
              "thinkdiff_hip::beam_select: top_lp must be a contiguous fp32 tensor of top_ids' shape on its device");
  for (const at::Tensor* t : {&rank_in, (const at::Tensor*)&token, (const at::Tensor*)&rank_out, (const at::Tensor*)&copy_src, (const at::Tensor*)&parent,
                              (const at::Tensor*)&fin_flag})
    TORCH_CHECK(t->device() == top_ids.device() && t->scalar_type() == at::kInt && t->is_contiguous() && t->numel() == rows,
                "thinkdiff_hip::beam_select: rank_in, token, rank_out, copy_src, parent and fin_flag must be contiguous int32 tensors of ", rows, " entries on top_ids' device");
  for (const at::Tensor* t : {&cum_in, (const at::Tensor*)&cum_out, (const at::Tensor*)&fin_cum})
    TORCH_CHECK(t->device() == top_ids.device() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == rows,
                "thinkdiff_hip::beam_select: cum_in, cum_out and fin_cum must be contiguous fp32 tensors of ", rows, " entries on top_ids' device");
  TORCH_CHECK(eos >= -1 && eos <= std::numeric_limits<int>::max(), "thinkdiff_hip::beam_select: eos=", eos, " is neither a token id nor -1");
  DeviceGuard guard(top_ids.device());
  ok(td_beam_select((const int32_t*)top_ids.data_ptr(), (const float*)top_lp.data_ptr(), (int)cap, (const float*)cum_in.data_ptr(), (const int32_t*)rank_in.data_ptr(),
                    (int)(rows / W), (int)W, (int)n_in, (int)eos, (int32_t*)token.data_ptr(), (float*)cum_out.data_ptr(), (int32_t*)rank_out.data_ptr(),
                    (int32_t*)copy_src.data_ptr(), (int32_t*)parent.data_ptr(), (int32_t*)fin_flag.data_ptr(), (float*)fin_cum.data_ptr(), stream_of(top_ids)));
}

// multi-row decode attention (td_attention_verify): q bf16 [R, Hq 128] (row stride free), the cache as k / v bf16 [slots, S, >= Hkv 128] views, or -- k_scale
// given -- k / v uint8 planes with k_scale / v_scale fp32 [slots, S, >= Hkv]; the four per-sequence int32 device tensors [n_seq] -> o bf16 [R, Hq 128]
at::Tensor attention_verify(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const c10::optional<at::Tensor>& k_scale,
                            const c10::optional<at::Tensor>& v_scale, const at::Tensor& seq_row0, const at::Tensor& seq_rows, const at::Tensor& seq_len0,
                            const at::Tensor& seq_slot, int64_t Hq, int64_t Hkv, double scale) {
  TORCH_CHECK(q.is_cuda(), "thinkdiff_hip: q must live on the GPU");
  const bool kv8 = k_scale.has_value();
  TORCH_CHECK(kv8 == v_scale.has_value(), "thinkdiff_hip::attention_verify: k_scale and v_scale come together (the e4m3 cache) or not at all (bf16)");
  TORCH_CHECK(q.dim() == 2 && q.scalar_type() == at::kBFloat16 && q.stride(1) == 1, "thinkdiff_hip::attention_verify: q must be bf16 [R, Hq x 128] with unit column stride");
  const auto kvt = kv8 ? at::kByte : at::kBFloat16;
  TORCH_CHECK(k.dim() == 3 && v.dim() == 3 && k.scalar_type() == kvt && v.scalar_type() == kvt && k.stride(2) == 1 && k.strides() == v.strides() && k.sizes() == v.sizes() &&
                  k.device() == q.device() && v.device() == q.device(),
              "thinkdiff_hip::attention_verify: k and v must be [slots, S, Hkv x 128] views of one shape and stride on q's device, bf16, or uint8 with scales");
  const int64_t n = seq_row0.numel();
  for (const at::Tensor* t : {&seq_row0, &seq_rows, &seq_len0, &seq_slot})
    TORCH_CHECK(t->device() == q.device() && t->scalar_type() == at::kInt && t->is_contiguous() && t->numel() == n,
                "thinkdiff_hip::attention_verify: seq_row0, seq_rows, seq_len0 and seq_slot must be contiguous int32 tensors of one length on q's device");
  const float *ks = nullptr, *vs = nullptr;
  int64_t lds = 0, sb = 0;
  if (kv8) {
    TORCH_CHECK(k_scale->dim() == 3 && k_scale->scalar_type() == at::kFloat && v_scale->scalar_type() == at::kFloat && k_scale->stride(2) == 1 &&
                    k_scale->strides() == v_scale->strides() && k_scale->device() == q.device() && v_scale->device() == q.device(),
                "thinkdiff_hip::attention_verify: k_scale and v_scale must be fp32 [slots, S, Hkv] views of one stride on q's device");
    ks = (const float*)k_scale->data_ptr(); vs = (const float*)v_scale->data_ptr(); lds = k_scale->stride(1); sb = k_scale->stride(0);
  }
  DeviceGuard guard(q.device());
  at::Tensor o = at::empty({q.size(0), Hq * 128}, q.options());
  ok(td_attention_verify(q.data_ptr(), q.stride(0), kv8 ? nullptr : k.data_ptr(), kv8 ? nullptr : v.data_ptr(), k.stride(1), k.stride(0), kv8 ? k.data_ptr() : nullptr,
                         kv8 ? v.data_ptr() : nullptr, ks, vs, lds, sb, o.data_ptr(), o.stride(0), (int)n, (const int32_t*)seq_row0.data_ptr(),
                         (const int32_t*)seq_rows.data_ptr(), (const int32_t*)seq_len0.data_ptr(), (const int32_t*)seq_slot.data_ptr(), (int)Hq, (int)Hkv, (float)scale,
                         stream_of(q)));
  return o;
}

// context attention (td_attention_prefix_segments_bf16): packed causal query segments q [R, >= Hq x 128] over key ranges of their own in k / v [rows, >= Hkv x 128]
// (views of one stride: a KV cache seen as rows); seg_starts int32 [n + 1], kv_row0 / kv_lens int32 [n] on q's device -> o [R, Hq x 128]
at::Tensor attention_prefix_segments(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const at::Tensor& seg_starts, const at::Tensor& kv_row0,
                                     const at::Tensor& kv_lens, int64_t max_q_len, int64_t max_kv_len, int64_t Hq, int64_t Hkv, double scale) {
  TORCH_CHECK(q.is_cuda(), "thinkdiff_hip: q must live on the GPU");
  TORCH_CHECK(q.dim() == 2 && q.scalar_type() == at::kBFloat16 && q.stride(1) == 1, "thinkdiff_hip::attention_prefix_segments: q must be bf16 [R, Hq x 128] with unit column stride");
  TORCH_CHECK(k.dim() == 2 && v.dim() == 2 && k.scalar_type() == at::kBFloat16 && v.scalar_type() == at::kBFloat16 && k.stride(1) == 1 && k.strides() == v.strides() &&
                  k.sizes() == v.sizes() && k.device() == q.device() && v.device() == q.device(),
              "thinkdiff_hip::attention_prefix_segments: k and v must be bf16 [rows, Hkv x 128] views of one shape and stride on q's device");
  const int64_t n = kv_row0.numel();
  for (const at::Tensor* t : {&seg_starts, &kv_row0, &kv_lens})
    TORCH_CHECK(t->device() == q.device() && t->scalar_type() == at::kInt && t->is_contiguous(),
                "thinkdiff_hip::attention_prefix_segments: seg_starts, kv_row0 and kv_lens must be contiguous int32 tensors on q's device");
  TORCH_CHECK(n >= 1 && kv_lens.numel() == n && seg_starts.numel() == n + 1, "thinkdiff_hip::attention_prefix_segments: seg_starts [n + 1], kv_row0 [n] and kv_lens [n] must pair up in length");
  DeviceGuard guard(q.device());
  at::Tensor o = at::empty({q.size(0), Hq * 128}, q.options());
  ok(td_attention_prefix_segments_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), q.stride(0), k.stride(0), o.stride(0), (const int*)seg_starts.data_ptr(),
                                       (const int*)kv_row0.data_ptr(), (const int*)kv_lens.data_ptr(), (int)n, (int)max_q_len, (int)max_kv_len, (int)Hq, (int)Hkv, (float)scale,
                                       stream_of(q)));
  return o;
}

// the accept rule of speculative decoding (td_spec_accept): sampled / fed int32 [R], seq_row0 / seq_rows int32 [B] -> (n_emit int32 [B], emit int32 [B, 8])
std::tuple<at::Tensor, at::Tensor> spec_accept(const at::Tensor& sampled, const at::Tensor& fed, const at::Tensor& seq_row0, const at::Tensor& seq_rows) {
  TORCH_CHECK(sampled.is_cuda(), "thinkdiff_hip: sampled must live on the GPU");
  const int64_t B = seq_row0.numel();
  for (const at::Tensor* t : {&sampled, &fed, &seq_row0, &seq_rows})
    TORCH_CHECK(t->device() == sampled.device() && t->scalar_type() == at::kInt && t->is_contiguous(),
                "thinkdiff_hip::spec_accept: sampled, fed, seq_row0 and seq_rows must be contiguous int32 tensors on one device");
  TORCH_CHECK(fed.numel() == sampled.numel() && seq_rows.numel() == B, "thinkdiff_hip::spec_accept: sampled / fed and seq_row0 / seq_rows must pair up in length");
  DeviceGuard guard(sampled.device());
  at::Tensor n_emit = at::empty({B}, sampled.options()), emit = at::empty({B, TD_MAX_VERIFY_ROWS}, sampled.options());
  ok(td_spec_accept((const int32_t*)sampled.data_ptr(), (const int32_t*)fed.data_ptr(), (const int32_t*)seq_row0.data_ptr(), (const int32_t*)seq_rows.data_ptr(), (int)B,
                    (int32_t*)n_emit.data_ptr(), (int32_t*)emit.data_ptr(), stream_of(sampled)));
  return {n_emit, emit};
}

}  // namespace

TORCH_LIBRARY(thinkdiff_hip, m) {
  m.def("linear(Tensor x, Tensor w, Tensor? bias, int act, Tensor? gate, Tensor? res) -> Tensor");
  m.def("aligner_mlp2x(Tensor x, Tensor w0, Tensor b0, Tensor w2, Tensor b2, Tensor norm_w, float eps, bool fp32_norm) -> Tensor");
  m.def("attention(Tensor q, Tensor k, Tensor v, int Hq, int Hkv, float scale, bool causal) -> Tensor");
  m.def("norm_rows(Tensor x, bool rms, float eps, Tensor? w, int split, Tensor? shiftA, Tensor? scaleA, Tensor? shiftB, Tensor? scaleB) -> Tensor");
  m.def("qk_norm_rope_(Tensor(a!) qkv, int Hq, int Hk, int q_col, int k_col, Tensor cos, Tensor sin, int split, Tensor? wqA, Tensor? wkA, Tensor? wqB, Tensor? wkB, float eps, bool rotate_half) -> Tensor(a!)");
  m.def("euler_step_(Tensor(a!) x, Tensor v, float dt) -> Tensor(a!)");
  m.def("flux_pack_latents(Tensor latents) -> Tensor");
  m.def("flux_unpack_latents(Tensor packed, int C, int H, int W, float div, float add) -> Tensor");
  m.def("cls_avgpool2(Tensor tokens) -> Tensor");
  m.def("sample_top_p(Tensor logits, float temperature, float top_p, int seed, int offset) -> Tensor");
  m.def("sample_rows(Tensor logits, Tensor params, Tensor offsets, int? state, bool update_state) -> Tensor");
  m.def("sample_rows_edit(Tensor logits, Tensor params, Tensor offsets, int? state, bool update_state, int? edits, Tensor? edit_slots) -> Tensor");
  m.def("logprobs_rows(Tensor logits, Tensor ids, Tensor n_top, int top_cap) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("flux_forward_(int engine, Tensor latents, int step, Tensor(a!) velocity) -> Tensor(a!)");
  m.def("flux_denoise_(int engine, Tensor(a!) latents, float[] sigmas) -> Tensor(a!)");
  m.def("flux_denoise_multi_(int[] engines, Tensor(a!)[] latents, float[] sigmas, int[] streams) -> ()");
  m.def("vae_decode_u8(int engine, Tensor packed, int h, int w, float scaling_factor, float shift_factor) -> Tensor");
  m.def("attention_fp8(Tensor q, Tensor k, Tensor v, int H, float scale) -> Tensor");
  m.def("vae_encode_moments(int engine, Tensor image, int H, int W) -> Tensor");
  m.def("vae_latents_from_moments(Tensor moments, Tensor? eps, Tensor? noise, float sigma, float scaling_factor, float shift_factor, int h, int w) -> Tensor");
  m.def("flux_inpaint_step_(Tensor(a!) x, Tensor v, Tensor image_latents, Tensor? noise, Tensor mask, float dt, float sigma_next) -> Tensor(a!)");
  m.def("flux_inpaint_mask(Tensor mask, int C) -> Tensor");
  m.def("flux_denoise_inpaint_(int engine, Tensor(a!) latents, float[] sigmas, Tensor image_latents, Tensor noise, Tensor mask) -> Tensor(a!)");
  m.def("flux_set_channel_condition(int engine, Tensor cond) -> ()");
  m.def("flux_set_reference_tokens(int engine, Tensor ref_latents, Tensor ref_ids) -> ()");
  m.def("flux_cfg_step_(Tensor(a!) x, Tensor v_pos, Tensor v_neg, float scale, float dt) -> Tensor(a!)");
  m.def("flux_residual_inject_(Tensor(a!) h, Tensor r, float scale) -> Tensor(a!)");
  m.def("flux_residual_inject_multi_(Tensor(a!) h, Tensor[] r, float[] scales) -> Tensor(a!)");
  m.def("block_cache_head(Tensor h1, Tensor h0, Tensor? r_prev) -> (Tensor, Tensor)");
  m.def("block_cache_tail(Tensor a, Tensor b) -> Tensor");
  m.def("flux_denoise_cfg_(int engine_pos, int engine_neg, Tensor(a!) latents, float[] sigmas, float scale) -> Tensor(a!)");
  m.def("vae_encode_moments_masked(int engine, Tensor image, Tensor mask, int H, int W) -> Tensor");
  m.def("flux_fill_condition(Tensor moments, Tensor? eps, Tensor mask, float scaling_factor, float shift_factor, int H, int W) -> Tensor");
  m.def("flux_denoise_multi_inpaint_(int[] engines, Tensor(a!)[] latents, float[] sigmas, Tensor[] image_latents, Tensor[] noise, Tensor[] mask, int[] streams) -> ()");
  m.def("lora_merge(Tensor w, Tensor[] A, Tensor[] B, float[] scales) -> Tensor");
  m.def("lora_merge_(Tensor(a!) w, Tensor[] A, Tensor[] B, float[] scales) -> Tensor(a!)");
  m.def("lora_rows_(Tensor x, Tensor row_adapter, Tensor[] A, Tensor[] B, int[] pair, float[] scales, Tensor(a!)[] ys) -> ()");
  m.def("redux_compose(Tensor? text, Tensor? image, float[] scales, int text_rows) -> Tensor");
  m.def("image_resize_u8(Tensor img, int out_h, int out_w, int resample, int? out_channels) -> Tensor");
  m.def("ip_attention(Tensor q, Tensor k, Tensor v, int H, Tensor? norm_w, float eps, float out_scale) -> Tensor");
  m.def("ip_attention_(Tensor(a!) o, Tensor q, Tensor k, Tensor v, int H, Tensor? norm_w, float eps, float out_scale, bool accumulate) -> Tensor(a!)");
  m.def("flux_ip_adapter_load_param(int engine, int slot, str name, Tensor data) -> ()");
  m.def("flux_set_ip_image_embeds(int engine, int slot, Tensor embeds) -> ()");
  m.def("flux_ip_read(int engine, int slot, int block, int which) -> Tensor");
  m.def("flux_read_param(int engine, str name) -> Tensor");
  m.def("flux_lora_load(int engine, str adapter, str param, Tensor A, Tensor B, float scale) -> ()");
  m.def("flux_lora_set_adapters(int engine, str[] names, float[] weights) -> ()");
  m.def("flux_lora_delete(int engine, str adapter) -> ()");
  m.def("quant_weight_rows_e4m3(Tensor w) -> (Tensor, Tensor, Tensor)");
  m.def("kv_quant_rows_e4m3(Tensor kv, int heads) -> (Tensor, Tensor, Tensor)");
  m.def("kv_dequant_rows_e4m3(Tensor q, Tensor scale) -> Tensor");
  m.def("attention_decode_kv8(Tensor q, Tensor k8, Tensor v8, Tensor k_scale, Tensor v_scale, Tensor? kv_lens, int Hq, int Hkv, float scale) -> Tensor");
  m.def("linear_w8(Tensor x, Tensor wq, Tensor w_scale, Tensor? bias, int act, Tensor? gate, Tensor? res) -> Tensor");
  m.def("quant_weight_rows_mxfp4(Tensor w) -> (Tensor, Tensor, Tensor)");
  m.def("dequant_rows_mxfp4(Tensor packed, Tensor scales) -> Tensor");
  m.def("linear_w4(Tensor x, Tensor packed, Tensor scales, Tensor? bias, int act, Tensor? gate, Tensor? res) -> Tensor");
  m.def("repack_int4(int layout, Tensor qweight, Tensor qzeros, Tensor scales, int group_size) -> (Tensor, Tensor, Tensor)");
  m.def("dequant_rows_int4(Tensor packed, Tensor scales, Tensor zeros, int group_size) -> Tensor");
  m.def("linear_i4(Tensor x, Tensor packed, Tensor scales, Tensor zeros, int group_size, Tensor? bias, int act, Tensor? gate, Tensor? res) -> Tensor");
  m.def("kv_fork_rows(Tensor(a!) plane, int slot_rows, int src_slot, int[] dst_slots, int n_rows) -> ()");
  m.def("kv_gather_rows(Tensor(a!) plane, int slot_rows, int[] slots, Tensor copy_src, int[] n_rows) -> ()");
  m.def("attention_verify(Tensor q, Tensor k, Tensor v, Tensor? k_scale, Tensor? v_scale, Tensor seq_row0, Tensor seq_rows, Tensor seq_len0, Tensor seq_slot, int Hq, int Hkv, float scale) -> Tensor");
  m.def("attention_prefix_segments(Tensor q, Tensor k, Tensor v, Tensor seg_starts, Tensor kv_row0, Tensor kv_lens, int max_q_len, int max_kv_len, int Hq, int Hkv, float scale) -> Tensor");
  m.def("spec_accept(Tensor sampled, Tensor fed, Tensor seq_row0, Tensor seq_rows) -> (Tensor, Tensor)");
  m.def("beam_select(Tensor top_ids, Tensor top_lp, Tensor cum_in, Tensor rank_in, int W, int n_in, int eos, Tensor(a!) token, Tensor(b!) cum_out, Tensor(c!) rank_out, Tensor(d!) copy_src, Tensor(e!) parent, Tensor(f!) fin_flag, Tensor(g!) fin_cum) -> ()");
}

TORCH_LIBRARY_IMPL(thinkdiff_hip, CUDA, m) {
  m.impl("linear", &linear);
  m.impl("aligner_mlp2x", &aligner_mlp2x);
  m.impl("attention", &attention);
  m.impl("norm_rows", &norm_rows);
  m.impl("qk_norm_rope_", &qk_norm_rope_);
  m.impl("euler_step_", &euler_step_);
  m.impl("flux_pack_latents", &flux_pack_latents);
  m.impl("flux_unpack_latents", &flux_unpack_latents);
  m.impl("cls_avgpool2", &cls_avgpool2);
  m.impl("sample_top_p", &sample_top_p);
  m.impl("sample_rows", &sample_rows);
  m.impl("sample_rows_edit", &sample_rows_edit);
  m.impl("logprobs_rows", &logprobs_rows);
  m.impl("flux_forward_", &flux_forward_);
  m.impl("flux_denoise_", &flux_denoise_);
  m.impl("flux_denoise_multi_", &flux_denoise_multi_);
  m.impl("vae_decode_u8", &vae_decode_u8);
  m.impl("attention_fp8", &attention_fp8);
  m.impl("vae_encode_moments", &vae_encode_moments);
  m.impl("vae_latents_from_moments", &vae_latents_from_moments);
  m.impl("flux_inpaint_step_", &flux_inpaint_step_);
  m.impl("flux_inpaint_mask", &flux_inpaint_mask);
  m.impl("flux_denoise_inpaint_", &flux_denoise_inpaint_);
  m.impl("flux_denoise_multi_inpaint_", &flux_denoise_multi_inpaint_);
  m.impl("flux_set_channel_condition", &flux_set_channel_condition);
  m.impl("flux_set_reference_tokens", &flux_set_reference_tokens);
  m.impl("flux_cfg_step_", &flux_cfg_step_);
  m.impl("flux_residual_inject_", &flux_residual_inject_);
  m.impl("flux_residual_inject_multi_", &flux_residual_inject_multi_);
  m.impl("block_cache_head", &block_cache_head);
  m.impl("block_cache_tail", &block_cache_tail);
  m.impl("flux_denoise_cfg_", &flux_denoise_cfg_);
  m.impl("vae_encode_moments_masked", &vae_encode_moments_masked);
  m.impl("flux_fill_condition", &flux_fill_condition);
  m.impl("lora_merge", &lora_merge);
  m.impl("lora_merge_", &lora_merge_);
  m.impl("lora_rows_", &lora_rows_);
  m.impl("flux_lora_load", &flux_lora_load);
  m.impl("redux_compose", &redux_compose);
  m.impl("image_resize_u8", &image_resize_u8);
  m.impl("ip_attention", &ip_attention);
  m.impl("ip_attention_", &ip_attention_);
  m.impl("flux_ip_adapter_load_param", &flux_ip_adapter_load_param);
  m.impl("flux_set_ip_image_embeds", &flux_set_ip_image_embeds);
  m.impl("quant_weight_rows_e4m3", &quant_weight_rows_e4m3);
  m.impl("kv_quant_rows_e4m3", &kv_quant_rows_e4m3);
  m.impl("kv_dequant_rows_e4m3", &kv_dequant_rows_e4m3);
  m.impl("attention_decode_kv8", &attention_decode_kv8);
  m.impl("linear_w8", &linear_w8);
  m.impl("quant_weight_rows_mxfp4", &quant_weight_rows_mxfp4);
  m.impl("dequant_rows_mxfp4", &dequant_rows_mxfp4);
  m.impl("linear_w4", &linear_w4);
  m.impl("repack_int4", &repack_int4);
  m.impl("dequant_rows_int4", &dequant_rows_int4);
  m.impl("linear_i4", &linear_i4);
  m.impl("kv_fork_rows", &kv_fork_rows);
  m.impl("kv_gather_rows", &kv_gather_rows);
  m.impl("beam_select", &beam_select);
  m.impl("attention_verify", &attention_verify);
  m.impl("attention_prefix_segments", &attention_prefix_segments);
  m.impl("spec_accept", &spec_accept);
}

TORCH_LIBRARY_IMPL(thinkdiff_hip, CompositeExplicitAutograd, m) {
  m.impl("flux_read_param", &flux_read_param);
  m.impl("flux_ip_read", &flux_ip_read);
  m.impl("flux_lora_set_adapters", &flux_lora_set_adapters);
  m.impl("flux_lora_delete", &flux_lora_delete);
}
