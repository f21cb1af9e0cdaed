// Torch bindings for fengshen_amd HIP kernels (gfx950).
// Kernels live in kernels.hip / flash_attn.hip as extern "C" launchers taking
// raw pointers + hipStream_t; this file owns all Tensor plumbing.
#include <torch/extension.h>

#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include <string>
#include <vector>

#include "flash_blockmap.h"
#include "flash_v3.h"

enum FsDtype { FS_F32 = 0, FS_BF16 = 1, FS_F16 = 2 };

static int fs_dtype(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return FS_F32;
    case at::kBFloat16: return FS_BF16;
    case at::kHalf: return FS_F16;
    default: TORCH_CHECK(false, "unsupported dtype ", t.scalar_type());
  }
}

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

extern "C" {
void fs_rms_norm_fwd(const void*, const void*, void*, float*, int, int, float,
                     int, hipStream_t);
void fs_rms_norm_bwd(const void*, const void*, const void*, const float*,
                     void*, float*, int, int, int, hipStream_t);
void fs_layer_norm_fwd(const void*, const void*, const void*, void*, float*,
                       float*, int, int, float, int, hipStream_t);
void fs_layer_norm_bwd(const void*, const void*, const void*, const float*,
                       const float*, void*, float*, float*, int, int, int,
                       hipStream_t);
void fs_scaled_softmax_fwd(const void*, const unsigned char*, void*, float,
                           int, int, int, int, int, int, int, int,
                           hipStream_t);
void fs_scaled_softmax_bwd(const void*, const void*, void*, float, int, int,
                           int, hipStream_t);
void fs_rope(const void*, void*, const float*, const float*, long, int, int,
             int, int, int, hipStream_t);
void fs_swiglu_fwd(const void*, void*, long, int, int, hipStream_t);
void fs_swiglu_bwd(const void*, const void*, void*, long, int, int,
                   hipStream_t);
void fs_swiglu_bwd_act(const void*, const void*, void*, void*, long, int, int,
                       hipStream_t);
void fs_bias_gelu(const void*, const void*, const void*, void*, long, int, int,
                  int, hipStream_t);
void fs_fused_adamw(float*, const void*, float*, float*, void*, long, float,
                    float, float, float, float, int, int, int, hipStream_t);
void fs_flash_attn_fwd(const void*, const void*, const void*, void*, float*,
                       const int*, int, int, int, int, int, int, float,
                       float, unsigned long long, hipStream_t);
void fs_flash_attn_bwd(const void*, const void*, const void*, const void*,
                       const void*, const float*, void*, void*, void*, float*,
                       const int*, int, int, int, int, int, int, float,
                       float, unsigned long long, hipStream_t);
void fs_bf16_gemv(const void*, const void*, void*, int, int, int,
                  hipStream_t);
void fs_add_rms_norm(const void*, const void*, const void*, void*, void*,
                     int, int, float, hipStream_t);
void fs_decode_attn_split(const void*, void*, void*, const float*,
                          const float*, const void*, int, float*, void*, int,
                          int, int, int, int, float, int, int, hipStream_t);
void fs_decode_attn_split_mt(const void*, void*, void*, const float*,
                             const float*, const void*, int, float*, void*,
                             int, int, int, int, int, int, float, int, int,
                             hipStream_t);
void fs_decode_attn_split_q8(const void*, void*, float*, void*, float*,
                             const float*, const float*, const void*, int,
                             float*, void*, int, int, int, int, int, float,
                             int, int, hipStream_t);
void fs_kv_quantize_int8(const void*, void*, float*, long, int, hipStream_t);
void fs_decode_attn(const void*, void*, void*, const float*, const float*,
                    const void*, void*, int, int, int, int, int, float, int,
                    hipStream_t);
void fs_w8_gemv(const void*, const float*, const void*, void*, int, int, int,
                hipStream_t);
void fs_decode_gemm(const void*, const float*, const void*, void*, int, int,
                    int, int, hipStream_t);
int fs_decode_gemm_w4_ksplit(int, int, int);
void fs_decode_gemm_w4(const void*, const void*, const void*, void*, float*,
                       int, int, int, int, int, int, hipStream_t);
void fs_vocab_ce_fwd(const void*, const long*, float*, float*, float*,
                     long, int, int, int, hipStream_t);
void fs_vocab_ce_bwd(const void*, const long*, const float*, const float*,
                     const float*, void*, long, int, int, int, hipStream_t);
void fs_rope_inplace(void*, void*, const float*, const float*, int, int, int,
                     int, long, long, long, int, int, int, hipStream_t);
int fs_fused_norm_vectors(int);
int fs_fused_norm_bwd_grid(int, int);
void fs_res_rms_norm_fwd(const void*, const void*, const void*, void*, void*,
                         float*, int, int, float, int, hipStream_t);
void fs_res_rms_norm_bwd(const void*, const void*, const void*, const void*,
                         const float*, void*, float*, void*, int, int, int,
                         hipStream_t);
void fs_sparse_flash_fwd(const void*, const void*, const void*, void*, float*,
                         const int*, const int*, const int*,
                         const unsigned char*, int, int, int, int, int, int,
                         float, hipStream_t);
void fs_sparse_flash_bwd(const void*, const void*, const void*, const void*,
                         const void*, const float*, void*, void*, void*,
                         float*, const int*, const int*, const int*,
                         const int*, const int*, const int*,
                         const unsigned char*, int, int, int, int, int, int,
                         float, hipStream_t);
}

// ---------------------------------------------------------------------------
static std::vector<at::Tensor> rms_norm_fwd(at::Tensor x, at::Tensor w,
                                            double eps) {
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous());
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden must be divisible by 8");
  const long rows = x.numel() / H;
  auto out = at::empty_like(x);
  auto invrms = at::empty({rows}, x.options().dtype(at::kFloat));
  fs_rms_norm_fwd(x.data_ptr(), w.data_ptr(), out.data_ptr(),
                  invrms.data_ptr<float>(), (int)rows, H, (float)eps,
                  fs_dtype(x), cur_stream());
  return {out, invrms};
}

static std::vector<at::Tensor> rms_norm_bwd(at::Tensor gy, at::Tensor x,
                                            at::Tensor w, at::Tensor invrms) {
  const int H = x.size(-1);
  const long rows = x.numel() / H;
  auto gx = at::empty_like(x);
  auto gw32 = at::zeros({H}, x.options().dtype(at::kFloat));
  fs_rms_norm_bwd(gy.data_ptr(), x.data_ptr(), w.data_ptr(),
                  invrms.data_ptr<float>(), gx.data_ptr(),
                  gw32.data_ptr<float>(), (int)rows, H, fs_dtype(x),
                  cur_stream());
  return {gx, gw32.to(w.scalar_type())};
}

// Dispatch branch of the residual RMSNorm entry points for hidden size H:
// "reg<vectors per thread>" for the register-resident kernels, "lds" for the
// fallback.
static std::string fused_norm_branch(int64_t H) {
  const int nv = fs_fused_norm_vectors((int)H);
  return nv ? "reg" + std::to_string(nv) : std::string("lds");
}

// (sum, h, invrms); sum = x + delta rounded to x's dtype, or x itself when
// delta is absent.  h is the RMSNorm of the rounded sum.
static std::vector<at::Tensor> residual_rms_norm_fwd(
    at::Tensor x, c10::optional<at::Tensor> delta, at::Tensor w, double eps) {
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous());
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden must be divisible by 8");
  TORCH_CHECK(w.numel() == H && w.scalar_type() == x.scalar_type());
  const bool has_delta = delta.has_value();
  if (has_delta)
    TORCH_CHECK(delta->is_contiguous() && delta->sizes() == x.sizes() &&
                delta->scalar_type() == x.scalar_type());
  if (fs_fused_norm_vectors(H) == 0) {
    at::Tensor sum = has_delta ? at::add(x, *delta) : x;
    auto r = rms_norm_fwd(sum, w, eps);
    return {sum, r[0], r[1]};
  }
  const long rows = x.numel() / H;
  at::Tensor sum = has_delta ? at::empty_like(x) : x;
  auto h = at::empty_like(x);
  auto invrms = at::empty({rows}, x.options().dtype(at::kFloat));
  fs_res_rms_norm_fwd(x.data_ptr(), has_delta ? delta->data_ptr() : nullptr,
                      w.data_ptr(), has_delta ? sum.data_ptr() : nullptr,
                      h.data_ptr(), invrms.data_ptr<float>(), (int)rows, H,
                      (float)eps, fs_dtype(x), cur_stream());
  return {sum, h, invrms};
}

// (g, gw); g = norm input gradient (+ g_res when given), gw in w's dtype.
static std::vector<at::Tensor> residual_rms_norm_bwd(
    at::Tensor g_h, c10::optional<at::Tensor> g_res, at::Tensor x,
    at::Tensor w, at::Tensor invrms) {
  TORCH_CHECK(g_h.is_contiguous() && x.is_contiguous() && w.is_contiguous());
  TORCH_CHECK(g_h.sizes() == x.sizes() &&
              g_h.scalar_type() == x.scalar_type());
  const int H = x.size(-1);
  const long rows = x.numel() / H;
  TORCH_CHECK(H % 8 == 0, "hidden must be divisible by 8");
  TORCH_CHECK(invrms.is_contiguous() && invrms.scalar_type() == at::kFloat &&
              invrms.numel() == rows, "invrms must be ", rows, " floats");
  TORCH_CHECK(w.numel() == H);
  const bool has_res = g_res.has_value();
  if (has_res)
    TORCH_CHECK(g_res->is_contiguous() && g_res->sizes() == x.sizes() &&
                g_res->scalar_type() == x.scalar_type());
  if (fs_fused_norm_vectors(H) == 0) {
    auto r = rms_norm_bwd(g_h, x, w, invrms);
    return {has_res ? at::add(r[0], *g_res) : r[0], r[1]};
  }
  TORCH_CHECK(w.scalar_type() == x.scalar_type());
  auto g = at::empty_like(x);
  auto gw = at::empty_like(w);
  auto part = at::empty({fs_fused_norm_bwd_grid((int)rows, H), H},
                        x.options().dtype(at::kFloat));
  fs_res_rms_norm_bwd(g_h.data_ptr(), has_res ? g_res->data_ptr() : nullptr,
                      x.data_ptr(), w.data_ptr(), invrms.data_ptr<float>(),
                      g.data_ptr(), part.data_ptr<float>(), gw.data_ptr(),
                      (int)rows, H, fs_dtype(x), cur_stream());
  return {g, gw};
}

static std::vector<at::Tensor> layer_norm_fwd(at::Tensor x, at::Tensor w,
                                              c10::optional<at::Tensor> b,
                                              double eps) {
  TORCH_CHECK(x.is_contiguous());
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden must be divisible by 8");
  const long rows = x.numel() / H;
  auto out = at::empty_like(x);
  auto mean = at::empty({rows}, x.options().dtype(at::kFloat));
  auto invstd = at::empty({rows}, x.options().dtype(at::kFloat));
  fs_layer_norm_fwd(x.data_ptr(), w.data_ptr(),
                    b.has_value() ? b->data_ptr() : nullptr, out.data_ptr(),
                    mean.data_ptr<float>(), invstd.data_ptr<float>(),
                    (int)rows, H, (float)eps, fs_dtype(x), cur_stream());
  return {out, mean, invstd};
}

static std::vector<at::Tensor> layer_norm_bwd(at::Tensor gy, at::Tensor x,
                                              at::Tensor w, at::Tensor mean,
                                              at::Tensor invstd) {
  const int H = x.size(-1);
  const long rows = x.numel() / H;
  auto gx = at::empty_like(x);
  auto gw32 = at::zeros({H}, x.options().dtype(at::kFloat));
  auto gb32 = at::zeros({H}, x.options().dtype(at::kFloat));
  fs_layer_norm_bwd(gy.data_ptr(), x.data_ptr(), w.data_ptr(),
                    mean.data_ptr<float>(), invstd.data_ptr<float>(),
                    gx.data_ptr(), gw32.data_ptr<float>(),
                    gb32.data_ptr<float>(), (int)rows, H, fs_dtype(x),
                    cur_stream());
  return {gx, gw32.to(w.scalar_type()), gb32.to(w.scalar_type())};
}

// x: [b, np, sq, sk]; mask: uint8/bool [mb, 1, sq, sk] (1 = masked)
static at::Tensor scaled_masked_softmax_fwd(at::Tensor x,
                                            c10::optional<at::Tensor> mask,
                                            double scale) {
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous());
  const int sk = x.size(3), sq = x.size(2), np = x.size(1), b = x.size(0);
  auto out = at::empty_like(x);
  const unsigned char* mp = nullptr;
  at::Tensor m8;
  int mb = 1, mode = 0, mask_sq = 1;
  if (mask.has_value()) {
    m8 = mask->to(at::kByte).contiguous();
    TORCH_CHECK(m8.dim() == 4 && m8.size(3) == sk &&
                    (m8.size(2) == sq || m8.size(2) == 1),
                "mask must be [mb,1,sq|1,sk]");
    mb = m8.size(0);
    mask_sq = m8.size(2);
    TORCH_CHECK(mb == 1 || mb == b, "mask batch must be 1 or b");
    mp = m8.data_ptr<unsigned char>();
    mode = 1;
  }
  fs_scaled_softmax_fwd(x.data_ptr(), mp, out.data_ptr(), (float)scale,
                        b * np * sq, sk, sq, np, mb, mask_sq, mode,
                        fs_dtype(x), cur_stream());
  return out;
}

// x: [ab, sq, sk] with sq == sk, causal mask generated in-kernel
static at::Tensor scaled_causal_softmax_fwd(at::Tensor x, double scale) {
  TORCH_CHECK(x.dim() == 3 && x.is_contiguous());
  const int sk = x.size(2), sq = x.size(1), ab = x.size(0);
  TORCH_CHECK(sq == sk, "causal softmax needs sq == sk");
  auto out = at::empty_like(x);
  fs_scaled_softmax_fwd(x.data_ptr(), nullptr, out.data_ptr(), (float)scale,
                        ab * sq, sk, sq, 1, 1, sq, 2, fs_dtype(x),
                        cur_stream());
  return out;
}

static at::Tensor scaled_softmax_bwd(at::Tensor gy, at::Tensor y,
                                     double scale) {
  TORCH_CHECK(gy.is_contiguous() && y.is_contiguous());
  const int sk = y.size(-1);
  const long rows = y.numel() / sk;
  auto gx = at::empty_like(y);
  fs_scaled_softmax_bwd(gy.data_ptr(), y.data_ptr(), gx.data_ptr(),
                        (float)scale, (int)rows, sk, fs_dtype(y),
                        cur_stream());
  return gx;
}

// q,k: [b, np, s, hn]; cos/sin: [S, hn] fp32
static std::vector<at::Tensor> rope_fwd(at::Tensor q, at::Tensor k,
                                        at::Tensor cos, at::Tensor sin,
                                        int64_t offset) {
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous());
  TORCH_CHECK(cos.scalar_type() == at::kFloat && cos.is_contiguous());
  const int hn = q.size(-1), s = q.size(-2);
  TORCH_CHECK((hn / 2) % 8 == 0, "head_dim/2 must be divisible by 8");
  auto qo = at::empty_like(q);
  auto ko = at::empty_like(k);
  const long bnq = q.numel() / ((long)s * hn);
  const long bnk = k.numel() / ((long)s * hn);
  fs_rope(q.data_ptr(), qo.data_ptr(), cos.data_ptr<float>(),
          sin.data_ptr<float>(), bnq, s, hn, (int)offset, 0, fs_dtype(q),
          cur_stream());
  fs_rope(k.data_ptr(), ko.data_ptr(), cos.data_ptr<float>(),
          sin.data_ptr<float>(), bnk, s, hn, (int)offset, 0, fs_dtype(k),
          cur_stream());
  return {qo, ko};
}

static std::vector<at::Tensor> rope_bwd(at::Tensor gq, at::Tensor gk,
                                        at::Tensor cos, at::Tensor sin,
                                        int64_t offset) {
  const int hn = gq.size(-1), s = gq.size(-2);
  auto qo = at::empty_like(gq);
  auto ko = at::empty_like(gk);
  const long bnq = gq.numel() / ((long)s * hn);
  const long bnk = gk.numel() / ((long)s * hn);
  fs_rope(gq.data_ptr(), qo.data_ptr(), cos.data_ptr<float>(),
          sin.data_ptr<float>(), bnq, s, hn, (int)offset, 1, fs_dtype(gq),
          cur_stream());
  fs_rope(gk.data_ptr(), ko.data_ptr(), cos.data_ptr<float>(),
          sin.data_ptr<float>(), bnk, s, hn, (int)offset, 1, fs_dtype(gk),
          cur_stream());
  return {qo, ko};
}

static at::Tensor swiglu_fwd(at::Tensor packed) {
  TORCH_CHECK(packed.is_contiguous());
  const int h2 = packed.size(-1);
  TORCH_CHECK(h2 % 16 == 0, "packed dim must be divisible by 16");
  const int h = h2 / 2;
  const long rows = packed.numel() / h2;
  auto sizes = packed.sizes().vec();
  sizes.back() = h;
  auto out = at::empty(sizes, packed.options());
  fs_swiglu_fwd(packed.data_ptr(), out.data_ptr(), rows, h, fs_dtype(packed),
                cur_stream());
  return out;
}

static at::Tensor swiglu_bwd(at::Tensor gy, at::Tensor packed) {
  const int h2 = packed.size(-1);
  const int h = h2 / 2;
  const long rows = packed.numel() / h2;
  auto gpacked = at::empty_like(packed);
  fs_swiglu_bwd(gy.contiguous().data_ptr(), packed.data_ptr(),
                gpacked.data_ptr(), rows, h, fs_dtype(packed), cur_stream());
  return gpacked;
}

// swiglu_bwd that also returns act = silu(gate) * up, bit for bit what
// swiglu_fwd(packed) returns.  gy: [..., h], packed: [..., 2h] -> (gpacked,
// act).  act_out may be omitted (allocated here) or given; it may be gy
// itself, in which case act overwrites gy in place: aliasing is allowed.
static std::vector<at::Tensor> swiglu_bwd_act(
    at::Tensor gy, at::Tensor packed, c10::optional<at::Tensor> act_out) {
  TORCH_CHECK(packed.is_cuda(), "packed must be a GPU tensor");
  TORCH_CHECK(packed.is_contiguous(), "packed must be contiguous");
  TORCH_CHECK(gy.is_contiguous(), "gy must be contiguous");
  TORCH_CHECK(gy.scalar_type() == packed.scalar_type(),
              "gy and packed must have the same dtype");
  TORCH_CHECK(packed.dim() >= 1 && packed.size(-1) % 16 == 0,
              "packed dim must be divisible by 16");
  const int h2 = packed.size(-1);
  const int h = h2 / 2;
  const long rows = packed.numel() / h2;
  auto sizes = packed.sizes().vec();
  sizes.back() = h;
  TORCH_CHECK(gy.sizes() == at::IntArrayRef(sizes),
              "gy must have packed's shape with half the last dim");
  at::Tensor act;
  if (act_out.has_value()) {
    act = *act_out;
    TORCH_CHECK(act.is_contiguous(), "act must be contiguous");
    TORCH_CHECK(act.scalar_type() == packed.scalar_type(),
                "act and packed must have the same dtype");
    TORCH_CHECK(act.device() == packed.device(),
                "act and packed must be on the same device");
    TORCH_CHECK(act.sizes() == at::IntArrayRef(sizes),
                "act must have packed's shape with half the last dim");
  } else {
    act = at::empty(sizes, packed.options());
  }
  TORCH_CHECK(gy.device() == packed.device(),
              "gy and packed must be on the same device");
  auto gpacked = at::empty_like(packed);
  if (rows > 0)
    fs_swiglu_bwd_act(gy.data_ptr(), packed.data_ptr(), gpacked.data_ptr(),
                      act.data_ptr(), rows, h, fs_dtype(packed), cur_stream());
  return {gpacked, act};
}

static at::Tensor bias_gelu_fwd(at::Tensor x, at::Tensor bias) {
  TORCH_CHECK(x.is_contiguous() && bias.is_contiguous());
  const int h = x.size(-1);
  TORCH_CHECK(h % 8 == 0);
  const long rows = x.numel() / h;
  auto out = at::empty_like(x);
  fs_bias_gelu(x.data_ptr(), bias.data_ptr(), nullptr, out.data_ptr(), rows, h,
               0, fs_dtype(x), cur_stream());
  return out;
}

static at::Tensor bias_gelu_bwd(at::Tensor gy, at::Tensor x, at::Tensor bias) {
  const int h = x.size(-1);
  const long rows = x.numel() / h;
  auto gx = at::empty_like(x);
  fs_bias_gelu(x.data_ptr(), bias.data_ptr(), gy.data_ptr(), gx.data_ptr(),
               rows, h, 1, fs_dtype(x), cur_stream());
  return gx;
}

static void fused_adamw(at::Tensor master, at::Tensor grad, at::Tensor m,
                        at::Tensor v, at::Tensor out_param, double lr,
                        double beta1, double beta2, double eps, double wd,
                        int64_t step) {
  TORCH_CHECK(master.scalar_type() == at::kFloat);
  TORCH_CHECK(master.is_contiguous() && grad.is_contiguous());
  void* outp = out_param.data_ptr() == master.data_ptr()
                   ? nullptr : out_param.data_ptr();
  fs_fused_adamw(master.data_ptr<float>(), grad.data_ptr(),
                 m.data_ptr<float>(), v.data_ptr<float>(), outp,
                 master.numel(), (float)lr, (float)beta1, (float)beta2,
                 (float)eps, (float)wd, (int)step, fs_dtype(grad),
                 outp ? fs_dtype(out_param) : FS_F32, cur_stream());
}

static const int kFlashDims[] = {40, 64, 80, 96, 128, 160};

static bool flash_dim_ok(int d) {
  for (int x : kFlashDims)
    if (x == d) return true;
  return false;
}

// q: [b, h, sq, d] bf16 contiguous; k,v: [b, h, sk, d].
// causal: sq == sk, sq % 64 == 0, klens must be absent.
// non-causal: cross-attention (sq != sk) and ragged sk allowed; optional
// klens int32 [b] = per-batch key length (suffix padding mask).
static std::vector<at::Tensor> flash_attn_fwd(
    at::Tensor q, at::Tensor k, at::Tensor v, double scale, bool causal,
    c10::optional<at::Tensor> klens, double drop_p, int64_t seed) {
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "flash_attn: bf16 only");
  TORCH_CHECK(q.dim() == 4 && flash_dim_ok(q.size(3)),
              "flash_attn: head_dim must be one of 40/64/80/96/128/160");
  const int b = q.size(0), h = q.size(1), sq = q.size(2), d = q.size(3);
  const int sk = k.size(2);
  if (causal) {
    TORCH_CHECK(sq == sk && sq % 64 == 0 && !klens.has_value(),
                "flash_attn causal: sq==sk, sq%64==0, no klens");
  } else {
    TORCH_CHECK(sq % 16 == 0 && sq >= 16,
                "flash_attn: sq must be a multiple of 16");
  }
  const int* klp = nullptr;
  if (klens.has_value()) {
    TORCH_CHECK(klens->scalar_type() == at::kInt && klens->numel() == b
                && klens->is_contiguous());
    klp = klens->data_ptr<int>();
  }
  auto o = at::empty_like(q);
  auto lse = at::empty({b, h, sq}, q.options().dtype(at::kFloat));
  fs_flash_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                    lse.data_ptr<float>(), klp, b, h, sq, sk, d,
                    causal ? 1 : 0, (float)scale, (float)drop_p,
                    (unsigned long long)seed, cur_stream());
  return {o, lse};
}

static std::vector<at::Tensor> flash_attn_bwd(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor dout,
    at::Tensor lse, double scale, bool causal,
    c10::optional<at::Tensor> klens, double drop_p, int64_t seed) {
  const int b = q.size(0), h = q.size(1), sq = q.size(2), d = q.size(3);
  const int sk = k.size(2);
  const int* klp = nullptr;
  if (klens.has_value()) klp = klens->data_ptr<int>();
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  auto delta = at::empty({b, h, sq}, q.options().dtype(at::kFloat));
  fs_flash_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                    dout.contiguous().data_ptr(), lse.data_ptr<float>(),
                    dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                    delta.data_ptr<float>(), klp, b, h, sq, sk, d,
                    causal ? 1 : 0, (float)scale, (float)drop_p,
                    (unsigned long long)seed, cur_stream());
  return {dq, dk, dv};
}

// --- strided v3 flash / in-place rotary -----------------------------------
// Operands are logical [b, h, s, d] bf16 views with arbitrary batch / head /
// row strides (e.g. thirds of a packed [b, s, 3*h*d] projection output).
// The kernels use 16-byte vector accesses, so the last dim must be
// unit-stride and every other stride and the base address 16-byte aligned.
// All of this is checked here, on the host, before anything is launched.
static void check_bf16_bhsd(const at::Tensor& t, const char* name, int b,
                            int h, int s, int d) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16, name,
              ": must be a bf16 GPU tensor");
  TORCH_CHECK(t.dim() == 4 && t.size(0) == b && t.size(1) == h &&
                  t.size(2) == s && t.size(3) == d,
              name, ": expected shape [", b, ", ", h, ", ", s, ", ", d, "]");
}

static void check_strided_view(const at::Tensor& t, const char* name, int b,
                               int h, int s, int d) {
  check_bf16_bhsd(t, name, b, h, s, d);
  TORCH_CHECK(t.stride(3) == 1, name, ": last dim must be unit-stride");
  for (int i = 0; i < 3; ++i)
    TORCH_CHECK(t.stride(i) > 0 && t.stride(i) % 8 == 0, name, ": stride ", i,
                " (", t.stride(i), ") must be a positive multiple of 8");
  TORCH_CHECK(t.storage_offset() % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, ": base offset must be a multiple of 8 elements");
  // the view must stay inside its storage
  const int64_t last = t.storage_offset() + (b - 1) * t.stride(0) +
                       (h - 1) * t.stride(1) + (s - 1) * t.stride(2) + d;
  TORCH_CHECK(last * 2 <= (int64_t)t.storage().nbytes(), name,
              ": view runs past its storage");
}

static void check_same_strides(const at::Tensor& a, const at::Tensor& b,
                               const char* what) {
  TORCH_CHECK(a.strides() == b.strides(), what, " must share strides");
}

static void strides3(const at::Tensor& t, long out[3]) {
  out[0] = t.stride(0);
  out[1] = t.stride(1);
  out[2] = t.stride(2);
}

// Grouped-query attention: k/v (and dk/dv) carry h_kv = k.size(1) heads,
// query head j uses KV head j / (h / h_kv).  Returns h_kv after checking
// what the GQA instantiations do not cover; h_kv == h takes none of this.
static int checked_kv_heads(const at::Tensor& k, int h, bool causal,
                            double drop_p, bool has_klens) {
  TORCH_CHECK(k.dim() == 4, "k must be [b, h_kv, s, d]");
  const int h_kv = k.size(1);
  if (h_kv == h) return h;
  TORCH_CHECK(h_kv >= 1 && h % h_kv == 0, "flash v3 GQA: ", h,
              " query heads are not a multiple of ", h_kv, " KV heads");
  TORCH_CHECK(causal, "flash v3 GQA: causal=True only");
  TORCH_CHECK(drop_p == 0.0, "flash v3 GQA: dropout is not supported");
  TORCH_CHECK(!has_klens, "flash v3 GQA: klens is not supported");
  return h_kv;
}

static const int* checked_klens(const c10::optional<at::Tensor>& klens,
                                bool causal, int b) {
  if (!klens.has_value()) return nullptr;
  TORCH_CHECK(!causal, "flash v3: klens only with causal=False");
  TORCH_CHECK(klens->is_cuda() && klens->scalar_type() == at::kInt &&
                  klens->numel() == b && klens->is_contiguous(),
              "flash v3: klens must be contiguous int32 [", b, "] on the GPU");
  return klens->data_ptr<int>();
}

// Per-row key start of the causal v3 kernels (ops/flash.py): kstart [b, s]
// int32, row i sees keys kstart[i] <= j <= i; qend [b, s/64] int32 is the
// query-loop bound of dkv (backward only).  Dtype, device, layout, shape
// and the options that exclude kstart are checked here, on the host, before
// anything is launched.  The kernels clamp what they read, so a bad value
// cannot move an address; check_values additionally copies both tensors to
// the host and verifies 0 <= kstart[i] <= i, that kstart is non-decreasing
// and that qend is the bound that follows from it.
static void check_kstart(const at::Tensor& kstart,
                         const c10::optional<at::Tensor>& qend, bool need_qend,
                         const at::Tensor& q, bool causal, double drop_p,
                         bool has_klens, bool check_values) {
  const int64_t b = q.size(0), s = q.size(2);
  TORCH_CHECK(causal, "flash v3: kstart needs causal=True");
  TORCH_CHECK(drop_p == 0.0, "flash v3: kstart does not support dropout");
  TORCH_CHECK(!has_klens, "flash v3: kstart and klens exclude each other");
  TORCH_CHECK(need_qend == qend.has_value(),
              need_qend ? "flash v3: backward with kstart needs qend"
                        : "flash v3: qend is a backward argument");
  TORCH_CHECK(kstart.scalar_type() == at::kInt, "flash v3: kstart must be int32");
  TORCH_CHECK(kstart.is_cuda() && kstart.device() == q.device(),
              "flash v3: kstart must be on the device of q");
  TORCH_CHECK(kstart.dim() == 2 && kstart.size(0) == b && kstart.size(1) == s,
              "flash v3: kstart must be [", b, ", ", s, "]");
  TORCH_CHECK(kstart.is_contiguous(), "flash v3: kstart must be contiguous");
  if (need_qend) {
    TORCH_CHECK(qend->scalar_type() == at::kInt, "flash v3: qend must be int32");
    TORCH_CHECK(qend->is_cuda() && qend->device() == q.device(),
                "flash v3: qend must be on the device of q");
    TORCH_CHECK(qend->dim() == 2 && qend->size(0) == b &&
                    qend->size(1) == s / 64,
                "flash v3: qend must be [", b, ", ", s / 64, "]");
    TORCH_CHECK(qend->is_contiguous(), "flash v3: qend must be contiguous");
  }
  if (!check_values) return;
  auto ks = kstart.cpu();
  const int* kp = ks.data_ptr<int>();
  for (int64_t bi = 0; bi < b; ++bi)
    for (int64_t i = 0; i < s; ++i) {
      const int v = kp[bi * s + i];
      TORCH_CHECK(v >= 0 && v <= i, "flash v3: kstart[", bi, ", ", i, "] = ",
                  v, " outside [0, ", i, "]");
      TORCH_CHECK(i == 0 || v >= kp[bi * s + i - 1], "flash v3: kstart[", bi,
                  "] decreases at ", i);
    }
  if (!need_qend) return;
  auto qe = qend->cpu();
  const int* ep = qe.data_ptr<int>();
  for (int64_t bi = 0; bi < b; ++bi) {
    int64_t i = 0;
    for (int64_t t = 0; t < s / 64; ++t) {
      while (i + 1 < s && kp[bi * s + i + 1] <= 64 * t + 63) ++i;
      TORCH_CHECK(ep[bi * (s / 64) + t] == i, "flash v3: qend[", bi, ", ", t,
                  "] = ", ep[bi * (s / 64) + t], ", expected ", i);
    }
  }
}

// Backward-only operands of a flash v3 call.
struct FlashV3Grads {
  const at::Tensor &dout, &lse, &dq, &dk, &dv;
};

// The one gate in front of the flash v3 launchers: checks every operand and
// option of a forward (g == nullptr) or backward call on the host, before
// anything is launched, and describes the call for fs_flash_v3_{fwd,bwd}
// (the caller adds the tensor it allocates: lse or delta_ws).  Strided
// entries take any view check_strided_view accepts.  Contiguous entries
// require is_contiguous() and derive the strides from the sizes, since a
// contiguous tensor may carry any stride on a size-1 dim.
static FlashV3Args checked_flash_v3(
    const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const at::Tensor& o, const FlashV3Grads* g, bool contiguous, double scale,
    bool causal, const c10::optional<at::Tensor>& klens, double drop_p,
    int64_t seed, const c10::optional<at::Tensor>& kstart,
    const c10::optional<at::Tensor>& qend, bool check_values) {
  TORCH_CHECK(q.dim() == 4, "q must be [b, h, s, d]");
  const int b = q.size(0), h = q.size(1), s = q.size(2), d = q.size(3);
  TORCH_CHECK((d == 128 || d == 96 || d == 64) && s % 64 == 0 && s >= 64,
              "flash v3: d in {64, 96, 128}, s a multiple of 64");
  const int h_kv = checked_kv_heads(k, h, causal, drop_p, klens.has_value());
  // checks t as a [b, heads, s, d] operand, writes its strides to st3 (if
  // given) and returns its address
  auto operand = [&](const at::Tensor& t, const char* name, int heads,
                     long* st3) {
    long st[3] = {(long)heads * s * d, (long)s * d, (long)d};
    if (contiguous) {
      check_bf16_bhsd(t, name, b, heads, s, d);
      TORCH_CHECK(t.is_contiguous(), name, ": must be contiguous");
      TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
                  ": base address must be 16-byte aligned");
    } else {
      check_strided_view(t, name, b, heads, s, d);
      strides3(t, st);
    }
    if (st3) std::copy(st, st + 3, st3);
    return t.data_ptr();
  };
  FlashV3Args a = {};
  a.q = operand(q, "q", h, a.qs);
  a.k = operand(k, "k", h_kv, a.kvs);
  a.v = operand(v, "v", h_kv, nullptr);
  a.o = operand(o, "o", h, a.os);
  // k|v (and dk|dv) share one stride triple; with h_kv == h it is q's (dq's)
  if (!contiguous) {
    if (h_kv == h) check_same_strides(q, k, "q and k");
    check_same_strides(k, v, "k and v");
  }
  if (g) {
    a.dout = operand(g->dout, "dout", h, a.dos);
    a.dq = operand(g->dq, "dq", h, a.gs);
    a.dk = operand(g->dk, "dk", h_kv, a.gkvs);
    a.dv = operand(g->dv, "dv", h_kv, nullptr);
    if (!contiguous) {
      if (h_kv == h) check_same_strides(g->dq, g->dk, "dq and dk");
      check_same_strides(g->dk, g->dv, "dk and dv");
    }
    TORCH_CHECK(g->lse.is_cuda() && g->lse.scalar_type() == at::kFloat &&
                    g->lse.is_contiguous() &&
                    g->lse.numel() == (int64_t)b * h * s,
                "lse must be contiguous fp32 [b, h, s]");
    a.lse = g->lse.data_ptr<float>();
  }
  if (kstart.has_value()) {
    check_kstart(*kstart, qend, g != nullptr, q, causal, drop_p,
                 klens.has_value(), check_values);
    a.kstart = kstart->data_ptr<int>();
    a.qend = g ? qend->data_ptr<int>() : nullptr;
  } else {
    TORCH_CHECK(!qend.has_value(), "flash v3: qend without kstart");
  }
  a.klens = checked_klens(klens, causal, b);
  a.b = b, a.h = h, a.h_kv = h_kv, a.s = s, a.d = d;
  a.causal = causal ? 1 : 0;
  a.scale = (float)scale;
  a.drop_p = (float)drop_p;
  a.seed = (unsigned long long)seed;
  return a;
}

// fp32 [b, h, s]: lse and the backward's delta scratch
static at::Tensor new_lse(const at::Tensor& q) {
  return at::empty({q.size(0), q.size(1), q.size(2)},
                   q.options().dtype(at::kFloat));
}

// Contiguous [b, h, s, d] operands (k, v: [b, h_kv, s, d]); returns (o, lse).
static std::vector<at::Tensor> flash_attn_fwd_v3(
    at::Tensor q, at::Tensor k, at::Tensor v, double scale, bool causal,
    c10::optional<at::Tensor> klens, double drop_p, int64_t seed,
    c10::optional<at::Tensor> kstart, bool check_values) {
  auto o = at::empty_like(q);
  FlashV3Args a =
      checked_flash_v3(q, k, v, o, nullptr, true, scale, causal, klens,
                       drop_p, seed, kstart, c10::nullopt, check_values);
  auto lse = new_lse(q);
  a.lse = lse.data_ptr<float>();
  fs_flash_v3_fwd(&a, cur_stream());
  return {o, lse};
}

// Returns (dq, dk, dv), contiguous.
static std::vector<at::Tensor> flash_attn_bwd_v3(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor dout,
    at::Tensor lse, double scale, bool causal,
    c10::optional<at::Tensor> klens, double drop_p, int64_t seed,
    c10::optional<at::Tensor> kstart, c10::optional<at::Tensor> qend,
    bool check_values) {
  dout = dout.contiguous();
  auto dq = at::empty_like(q), dk = at::empty_like(k), dv = at::empty_like(v);
  const FlashV3Grads g{dout, lse, dq, dk, dv};
  FlashV3Args a =
      checked_flash_v3(q, k, v, o, &g, true, scale, causal, klens, drop_p,
                       seed, kstart, qend, check_values);
  auto delta = new_lse(q);
  a.delta_ws = delta.data_ptr<float>();
  fs_flash_v3_bwd(&a, cur_stream());
  return {dq, dk, dv};
}

// Writes o in place; returns lse [b, h, s] fp32.  No dropout.
static at::Tensor flash_attn_fwd_v3_strided(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, double scale,
    bool causal, c10::optional<at::Tensor> klens,
    c10::optional<at::Tensor> kstart, bool check_values) {
  FlashV3Args a =
      checked_flash_v3(q, k, v, o, nullptr, false, scale, causal, klens, 0.0,
                       0, kstart, c10::nullopt, check_values);
  auto lse = new_lse(q);
  a.lse = lse.data_ptr<float>();
  fs_flash_v3_fwd(&a, cur_stream());
  return lse;
}

// Writes dq, dk, dv in place.
static void flash_attn_bwd_v3_strided(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor dout,
    at::Tensor lse, at::Tensor dq, at::Tensor dk, at::Tensor dv, double scale,
    bool causal, c10::optional<at::Tensor> klens,
    c10::optional<at::Tensor> kstart, c10::optional<at::Tensor> qend,
    bool check_values) {
  const FlashV3Grads g{dout, lse, dq, dk, dv};
  FlashV3Args a =
      checked_flash_v3(q, k, v, o, &g, false, scale, causal, klens, 0.0, 0,
                       kstart, qend, check_values);
  auto delta = new_lse(q);
  a.delta_ws = delta.data_ptr<float>();
  fs_flash_v3_bwd(&a, cur_stream());
}

// Host only: row L of the int32 [nx * ny * nz, 3] result is the logical
// (x, y, z) that the flash v3 kernels give the block with hardware linear id
// L, from the function the kernels call (flash_blockmap.h).
static at::Tensor flash_v3_block_map(int64_t nx, int64_t ny, int64_t nz,
                                     bool heavy_last) {
  TORCH_CHECK(nx >= 1 && ny >= 1 && nz >= 1 && nx * ny * nz <= (1 << 24),
              "flash_v3_block_map: grid (", nx, ", ", ny, ", ", nz, ")");
  const int64_t T = nx * ny * nz;
  auto out = at::empty({T, 3}, at::TensorOptions().dtype(at::kInt));
  int* p = out.data_ptr<int>();
  for (int64_t L = 0; L < T; ++L) {
    const FlashBlock blk = flash_v3_block_of(
        (unsigned int)L, (unsigned int)nx, (unsigned int)ny, (unsigned int)nz,
        heavy_last);
    p[3 * L + 0] = (int)blk.x;
    p[3 * L + 1] = (int)blk.y;
    p[3 * L + 2] = (int)blk.z;
  }
  return out;
}

// cos/sin tables of the in-place rotary: contiguous fp32 [S, hn] on the GPU
// with S >= offset + s.
static void check_rope_tables(const at::Tensor& cos, const at::Tensor& sin,
                              int64_t offset, int s, int hn) {
  TORCH_CHECK(cos.is_cuda() && sin.is_cuda() &&
              cos.scalar_type() == at::kFloat &&
              sin.scalar_type() == at::kFloat && cos.is_contiguous() &&
              sin.is_contiguous() && cos.dim() == 2 && cos.size(1) == hn &&
              sin.sizes() == cos.sizes(),
              "cos/sin must be contiguous fp32 [S, hn]");
  TORCH_CHECK(offset >= 0 && offset + s <= cos.size(0),
              "rope table too short for offset + s");
}

// Rotates q and k ([b, np, s, hn] views sharing strides) in place;
// bwd = transpose rotation for gradients.  cos/sin: [S, hn] fp32.
static void rope_inplace(at::Tensor q, at::Tensor k, at::Tensor cos,
                         at::Tensor sin, int64_t offset, bool bwd) {
  TORCH_CHECK(q.dim() == 4, "q must be [b, np, s, hn]");
  const int b = q.size(0), np = q.size(1), s = q.size(2), hn = q.size(3);
  TORCH_CHECK((hn / 2) % 8 == 0 && hn % 2 == 0,
              "head_dim/2 must be divisible by 8");
  check_strided_view(q, "q", b, np, s, hn);
  check_strided_view(k, "k", b, np, s, hn);
  check_same_strides(q, k, "q and k");
  check_rope_tables(cos, sin, offset, s, hn);
  fs_rope_inplace(q.data_ptr(), k.data_ptr(), cos.data_ptr<float>(),
                  sin.data_ptr<float>(), b, np, s, hn, q.stride(0),
                  q.stride(1), q.stride(2), (int)offset, bwd ? 1 : 0,
                  fs_dtype(q), cur_stream());
}

// One-tensor form: x is any [b, n, s, hn] view, e.g. the h + h_kv adjacent
// q and k heads of a grouped-query packed buffer.
static void rope_inplace_one(at::Tensor x, at::Tensor cos, at::Tensor sin,
                             int64_t offset, bool bwd) {
  TORCH_CHECK(x.dim() == 4, "x must be [b, n, s, hn]");
  const int b = x.size(0), np = x.size(1), s = x.size(2), hn = x.size(3);
  TORCH_CHECK((hn / 2) % 8 == 0 && hn % 2 == 0,
              "head_dim/2 must be divisible by 8");
  check_strided_view(x, "x", b, np, s, hn);
  check_rope_tables(cos, sin, offset, s, hn);
  fs_rope_inplace(x.data_ptr(), nullptr, cos.data_ptr<float>(),
                  sin.data_ptr<float>(), b, np, s, hn, x.stride(0),
                  x.stride(1), x.stride(2), (int)offset, bwd ? 1 : 0,
                  fs_dtype(x), cur_stream());
}

// x [b, in] bf16, q8 [out, in] int8, scale [out] fp32 -> y [b, out] bf16
static at::Tensor w8_gemv(at::Tensor q8, at::Tensor scale, at::Tensor x) {
  TORCH_CHECK(q8.scalar_type() == at::kChar && x.scalar_type() == at::kBFloat16);
  TORCH_CHECK(q8.is_contiguous() && x.is_contiguous());
  const int out = q8.size(0), in = q8.size(1);
  TORCH_CHECK(in % 16 == 0, "in_features must be divisible by 16");
  const int b = x.numel() / in;
  auto y = at::empty({b, out}, x.options());
  fs_w8_gemv(q8.data_ptr(), scale.data_ptr<float>(), x.data_ptr(),
             y.data_ptr(), b, in, out, cur_stream());
  return y;
}

// x [b, in] bf16 (b <= 8), w [out, in] bf16 -> y [b, out] bf16
static at::Tensor bf16_gemv(at::Tensor w, at::Tensor x) {
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 &&
              x.scalar_type() == at::kBFloat16);
  TORCH_CHECK(w.is_contiguous() && x.is_contiguous());
  const int out = w.size(0), in = w.size(1);
  TORCH_CHECK(in % 16 == 0, "in_features must be divisible by 16");
  const int b = x.numel() / in;
  TORCH_CHECK(b >= 1 && b <= 8, "bf16_gemv: batch must be 1..8");
  auto y = at::empty({b, out}, x.options());
  fs_bf16_gemv(w.data_ptr(), x.data_ptr(), y.data_ptr(), b, in, out,
               cur_stream());
  return y;
}

// Weight-streaming MFMA GEMM for 1..16 rows (decode_gemm.hip):
// w [out, K] bf16, or int8 with scale [out] fp32; x [..., K] bf16 with 1..16
// rows -> y [rows, out] bf16.  Allocates nothing but y.
static at::Tensor decode_gemm(at::Tensor w, at::Tensor x,
                              c10::optional<at::Tensor> scale) {
  const bool w8 = w.scalar_type() == at::kChar;
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous() &&
                  (w8 || w.scalar_type() == at::kBFloat16),
              "decode_gemm: w must be contiguous 2-D bf16 or int8");
  const int64_t out = w.size(0), K = w.size(1);
  TORCH_CHECK(out >= 1 && out < (1LL << 31) && K >= 64 && K < (1LL << 31) &&
                  K % 64 == 0,
              "decode_gemm: w must be [out >= 1, K] with K a positive "
              "multiple of 64, got [", out, ", ", K, "]");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.is_contiguous() &&
                  x.dim() >= 1 && x.size(-1) == K,
              "decode_gemm: x must be contiguous bf16 [..., ", K, "]");
  const int64_t rows = x.numel() / K;
  TORCH_CHECK(rows >= 1 && rows <= 16,
              "decode_gemm: x must have 1..16 rows, got ", rows);
  TORCH_CHECK(scale.has_value() == w8,
              "decode_gemm: scale must be given exactly when w is int8");
  if (w8)
    TORCH_CHECK(scale->scalar_type() == at::kFloat && scale->is_contiguous() &&
                    scale->dim() == 1 && scale->size(0) == out &&
                    scale->is_cuda() && scale->device() == w.device(),
                "decode_gemm: scale must be contiguous fp32 [", out,
                "] on w's device");
  TORCH_CHECK(w.is_cuda() && x.is_cuda() && x.device() == w.device(),
              "decode_gemm: w and x must be on the same GPU");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(w.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0,
              "decode_gemm: w and x must be 16-byte aligned");
  auto y = at::empty({rows, out}, x.options());
  fs_decode_gemm(w.data_ptr(), w8 ? scale->data_ptr<float>() : nullptr,
                 x.data_ptr(), y.data_ptr(), (int)rows, (int)K, (int)out,
                 w8 ? 1 : 0, cur_stream());
  return y;
}

// Split-K MFMA GEMM for int4 weights and 1..16 rows (decode_gemm_w4.hip):
// qweight uint8 [out_pad/16, K/128, 64, 16] and scales bf16 [K/128, out_pad]
// as utils/quantize.py: pack_int4 writes them; x [..., K] bf16 with 1..16
// rows -> y [rows, out] bf16.  ksplit = 0 lets the kernel's rule choose (a
// function of K and out_pad only); tw = 0 is the default tiles-per-wave
// build, 1 and 2 pick one.  Allocates y and, for ksplit > 1, the fp32
// partials, both from the current stream's allocator.
static at::Tensor decode_gemm_w4(at::Tensor qweight, at::Tensor scales,
                                 at::Tensor x, int64_t out, int64_t ksplit,
                                 int64_t tw) {
  TORCH_CHECK(qweight.scalar_type() == at::kByte && qweight.dim() == 4 &&
                  qweight.is_contiguous() && qweight.size(0) >= 4 &&
                  qweight.size(0) % 4 == 0 && qweight.size(1) >= 1 &&
                  qweight.size(2) == 64 && qweight.size(3) == 16,
              "decode_gemm_w4: qweight must be contiguous uint8 "
              "[out_pad/16, K/128, 64, 16] with out_pad a multiple of 64");
  const int64_t ng = qweight.size(1), out_pad = qweight.size(0) * 16;
  const int64_t K = ng * 128;
  TORCH_CHECK(out_pad < (1LL << 31) && K < (1LL << 31),
              "decode_gemm_w4: out_pad and K must be below 2^31");
  TORCH_CHECK(scales.scalar_type() == at::kBFloat16 && scales.dim() == 2 &&
                  scales.is_contiguous() && scales.size(0) == ng &&
                  scales.size(1) == out_pad,
              "decode_gemm_w4: scales must be contiguous bf16 [", ng, ", ",
              out_pad, "]");
  TORCH_CHECK(out >= 1 && out <= out_pad, "decode_gemm_w4: out must be in 1..",
              out_pad, ", got ", out);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.is_contiguous() &&
                  x.dim() >= 1 && x.size(-1) == K,
              "decode_gemm_w4: x must be contiguous bf16 [..., ", K, "]");
  const int64_t rows = x.numel() / K;
  TORCH_CHECK(rows >= 1 && rows <= 16,
              "decode_gemm_w4: x must have 1..16 rows, got ", rows);
  TORCH_CHECK(qweight.is_cuda() && x.is_cuda() && scales.is_cuda() &&
                  x.device() == qweight.device() &&
                  scales.device() == qweight.device(),
              "decode_gemm_w4: qweight, scales and x must be on the same GPU");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(qweight.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(scales.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0,
              "decode_gemm_w4: qweight, scales and x must be 16-byte aligned");
  TORCH_CHECK(ksplit >= 0 && ksplit <= ng,
              "decode_gemm_w4: ksplit must be in 0..K/128 = ", ng, ", got ",
              ksplit);
  TORCH_CHECK(tw >= 0 && tw <= 2, "decode_gemm_w4: tw must be 0, 1 or 2");
  if (ksplit == 0)
    ksplit = fs_decode_gemm_w4_ksplit((int)K, (int)out_pad, (int)tw);
  auto y = at::empty({rows, out}, x.options());
  at::Tensor part;
  if (ksplit > 1)
    part = at::empty({ksplit, rows, out_pad}, x.options().dtype(at::kFloat));
  fs_decode_gemm_w4(qweight.data_ptr(), scales.data_ptr(), x.data_ptr(),
                    y.data_ptr(), ksplit > 1 ? part.data_ptr<float>() : nullptr,
                    (int)rows, (int)K, (int)out, (int)out_pad, (int)ksplit,
                    (int)tw, cur_stream());
  return y;
}

// Fused decode step: qkv [b, (nh + 2*nkv)*d] bf16, kc/vc [b, nkv, L, d] bf16
// caches (written in-place at pos), cos/sin [max_len, d] fp32, pos [1] long.
// nkv comes from the caches and nh from the width of qkv (nkv == nh: plain
// multi-head attention).  Returns ctx [b, nh*d] bf16.
static at::Tensor decode_attn(at::Tensor qkv, at::Tensor kc, at::Tensor vc,
                              at::Tensor cos_t, at::Tensor sin_t,
                              at::Tensor pos, double scale, bool rope) {
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 && qkv.is_contiguous());
  TORCH_CHECK(kc.is_contiguous() && vc.is_contiguous());
  TORCH_CHECK(cos_t.scalar_type() == at::kFloat &&
              sin_t.scalar_type() == at::kFloat);
  TORCH_CHECK(pos.scalar_type() == at::kLong);
  TORCH_CHECK(kc.dim() == 4 && vc.sizes() == kc.sizes() &&
                  kc.scalar_type() == at::kBFloat16 &&
                  vc.scalar_type() == at::kBFloat16,
              "decode_attn: caches must be bf16 [b, nkv, L, d] of one shape");
  const int b = kc.size(0), nkv = kc.size(1), L = kc.size(2), d = kc.size(3);
  TORCH_CHECK(d == 64 || d == 128, "decode_attn: head dim must be 64/128");
  const int64_t w = qkv.numel() / b - 2 * (int64_t)nkv * d;  // nh * d
  TORCH_CHECK(qkv.numel() % b == 0 && w > 0 && w % d == 0 &&
                  (w / d) % nkv == 0,
              "decode_attn: qkv must be [b, (nh + 2*nkv)*d] with nh a "
              "multiple of the caches' ", nkv, " KV heads");
  const int nh = w / d;
  auto ctx = at::empty({b, nh * d}, qkv.options());
  fs_decode_attn(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                 cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
                 pos.data_ptr(), ctx.data_ptr(), b, nh, nkv, d, L,
                 (float)scale, rope ? 1 : 0, cur_stream());
  return ctx;
}

// Split-KV grouped decode step (decode_attn.hip).  Arguments as decode_attn,
// except pos: int64 [b] (per sequence) or [1] (broadcast), and nsplit: the
// number of chunks the key prefix of a row is split into (0 = automatic).
// The automatic count depends on shapes only, so a captured graph keeps it:
// the smallest nsplit that gives the grid two blocks per CU (256 CUs), capped
// at ceil(L / 256) and at 64.
// tokens = T in [2, 16] is the multi-token step (decode_attn_mt.hip): qkv is
// [b, T, (nh + 2*nkv)*d], token t of sequence b sits at pos_b + t, rows
// pos_b .. pos_b+T-1 of the caches are written, pos is clamped into
// [0, L - T] and the result is [b, T, nh*d].  The automatic nsplit counts
// ceil(T*G/16) column groups per KV head.  tokens = 1 is the call above.
static at::Tensor decode_attn_split(at::Tensor qkv, at::Tensor kc,
                                    at::Tensor vc, at::Tensor cos_t,
                                    at::Tensor sin_t, at::Tensor pos,
                                    double scale, bool rope, int64_t nsplit,
                                    int64_t tokens) {
  TORCH_CHECK(tokens >= 1 && tokens <= 16,
              "decode_attn_split: tokens must be in [1, 16], got ", tokens);
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 && qkv.is_contiguous(),
              "decode_attn_split: qkv must be contiguous bf16");
  TORCH_CHECK(kc.dim() == 4 && vc.sizes() == kc.sizes() &&
                  kc.scalar_type() == at::kBFloat16 &&
                  vc.scalar_type() == at::kBFloat16 && kc.is_contiguous() &&
                  vc.is_contiguous(),
              "decode_attn_split: caches must be contiguous bf16 "
              "[b, nkv, L, d] of one shape");
  const int b = kc.size(0), nkv = kc.size(1), L = kc.size(2), d = kc.size(3);
  TORCH_CHECK(d == 64 || d == 96 || d == 128,
              "decode_attn_split: head dim must be 64/96/128, got ", d);
  TORCH_CHECK(b >= 1 && nkv >= 1 && L >= 1 &&
                  qkv.numel() % (b * tokens) == 0,
              "decode_attn_split: empty cache or qkv not [b, ...]");
  TORCH_CHECK(tokens == 1 ||
                  (qkv.dim() == 3 && qkv.size(0) == b &&
                   qkv.size(1) == tokens && L >= tokens),
              "decode_attn_split: tokens = ", tokens, " needs qkv [", b, ", ",
              tokens, ", (nh + 2*nkv)*d] and a cache of at least ", tokens,
              " rows");
  // nh * d, per token
  const int64_t w = qkv.numel() / (b * tokens) - 2 * (int64_t)nkv * d;
  TORCH_CHECK(w > 0 && w % d == 0 && (w / d) % nkv == 0,
              "decode_attn_split: qkv must be [b, (nh + 2*nkv)*d] with nh a "
              "multiple of the caches' ", nkv, " KV heads");
  const int nh = w / d;
  TORCH_CHECK(pos.scalar_type() == at::kLong && pos.is_contiguous() &&
                  (pos.numel() == 1 || pos.numel() == b),
              "decode_attn_split: pos must be int64 with 1 or ", b,
              " elements");
  TORCH_CHECK(cos_t.scalar_type() == at::kFloat &&
                  sin_t.scalar_type() == at::kFloat && cos_t.dim() == 2 &&
                  sin_t.sizes() == cos_t.sizes() && cos_t.is_contiguous() &&
                  sin_t.is_contiguous() && cos_t.size(0) >= L &&
                  cos_t.size(1) == d,
              "decode_attn_split: cos/sin must be contiguous fp32 [>= ", L,
              ", ", d, "]");
  TORCH_CHECK(nsplit >= 0 && nsplit <= 64,
              "decode_attn_split: nsplit must be in [0, 64], got ", nsplit);
  TORCH_CHECK(qkv.is_cuda() && kc.is_cuda() && vc.is_cuda() &&
                  cos_t.is_cuda() && sin_t.is_cuda() && pos.is_cuda(),
              "decode_attn_split: all tensors must be on the GPU");
  if (nsplit == 0) {
    const int64_t blocks =
        (int64_t)b * nkv * ((tokens * (nh / nkv) + 15) / 16);
    nsplit = (2 * 256 + blocks - 1) / blocks;
    nsplit = std::min<int64_t>(nsplit, (L + 255) / 256);
    nsplit = std::max<int64_t>(std::min<int64_t>(nsplit, 64), 1);
  }
  if (tokens > 1) {
    auto ctx = at::empty({b, tokens, nh * d}, qkv.options());
    at::Tensor ws;
    if (nsplit > 1)
      ws = at::empty({b, tokens, nh, nsplit, d + 2},
                     qkv.options().dtype(at::kFloat));
    fs_decode_attn_split_mt(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                            cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
                            pos.data_ptr(), (int)pos.numel(),
                            nsplit > 1 ? ws.data_ptr<float>() : nullptr,
                            ctx.data_ptr(), b, (int)tokens, nh, nkv, d, L,
                            (float)scale, rope ? 1 : 0, (int)nsplit,
                            cur_stream());
    return ctx;
  }
  auto ctx = at::empty({b, nh * d}, qkv.options());
  at::Tensor ws;
  if (nsplit > 1)
    ws = at::empty({b, nh, nsplit, d + 2}, qkv.options().dtype(at::kFloat));
  fs_decode_attn_split(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                       cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
                       pos.data_ptr(), (int)pos.numel(),
                       nsplit > 1 ? ws.data_ptr<float>() : nullptr,
                       ctx.data_ptr(), b, nh, nkv, d, L, (float)scale,
                       rope ? 1 : 0, (int)nsplit, cur_stream());
  return ctx;
}

// decode_attn_split over an int8 KV cache (decode_attn_q8.hip).  kq/vq are
// int8 [b, nkv, L, d] with one fp32 scale per row in k_scale/v_scale
// [b, nkv, L]; row pos_b of all four is written here.  The other arguments
// and the automatic nsplit are those of decode_attn_split.  L must be a
// multiple of 4: the kernel reads the scales of 4 keys as one 16-byte load.
static at::Tensor decode_attn_split_q8(at::Tensor qkv, at::Tensor kq,
                                       at::Tensor k_scale, at::Tensor vq,
                                       at::Tensor v_scale, at::Tensor cos_t,
                                       at::Tensor sin_t, at::Tensor pos,
                                       double scale, bool rope,
                                       int64_t nsplit) {
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 && qkv.is_contiguous(),
              "decode_attn_split_q8: qkv must be contiguous bf16");
  TORCH_CHECK(kq.dim() == 4 && vq.sizes() == kq.sizes() &&
                  kq.scalar_type() == at::kChar &&
                  vq.scalar_type() == at::kChar && kq.is_contiguous() &&
                  vq.is_contiguous(),
              "decode_attn_split_q8: caches must be contiguous int8 "
              "[b, nkv, L, d] of one shape");
  const int b = kq.size(0), nkv = kq.size(1), L = kq.size(2), d = kq.size(3);
  TORCH_CHECK(d == 64 || d == 128,
              "decode_attn_split_q8: head dim must be 64 or 128, got ", d);
  TORCH_CHECK(b >= 1 && nkv >= 1 && L >= 4 && L % 4 == 0 &&
                  qkv.numel() % b == 0,
              "decode_attn_split_q8: cache length must be a positive "
              "multiple of 4 and qkv [b, ...]");
  TORCH_CHECK(k_scale.scalar_type() == at::kFloat &&
                  v_scale.scalar_type() == at::kFloat &&
                  k_scale.is_contiguous() && v_scale.is_contiguous() &&
                  k_scale.sizes() == kq.sizes().slice(0, 3) &&
                  v_scale.sizes() == kq.sizes().slice(0, 3),
              "decode_attn_split_q8: scales must be contiguous fp32 [", b,
              ", ", nkv, ", ", L, "]");
  const int64_t w = qkv.numel() / b - 2 * (int64_t)nkv * d;  // nh * d
  TORCH_CHECK(w > 0 && w % d == 0 && (w / d) % nkv == 0,
              "decode_attn_split_q8: qkv must be [b, (nh + 2*nkv)*d] with nh "
              "a multiple of the caches' ", nkv, " KV heads");
  const int nh = w / d;
  TORCH_CHECK(pos.scalar_type() == at::kLong && pos.is_contiguous() &&
                  (pos.numel() == 1 || pos.numel() == b),
              "decode_attn_split_q8: pos must be int64 with 1 or ", b,
              " elements");
  TORCH_CHECK(cos_t.scalar_type() == at::kFloat &&
                  sin_t.scalar_type() == at::kFloat && cos_t.dim() == 2 &&
                  sin_t.sizes() == cos_t.sizes() && cos_t.is_contiguous() &&
                  sin_t.is_contiguous() && cos_t.size(0) >= L &&
                  cos_t.size(1) == d,
              "decode_attn_split_q8: cos/sin must be contiguous fp32 [>= ", L,
              ", ", d, "]");
  TORCH_CHECK(nsplit >= 0 && nsplit <= 64,
              "decode_attn_split_q8: nsplit must be in [0, 64], got ", nsplit);
  TORCH_CHECK(qkv.is_cuda() && kq.is_cuda() && vq.is_cuda() &&
                  k_scale.is_cuda() && v_scale.is_cuda() && cos_t.is_cuda() &&
                  sin_t.is_cuda() && pos.is_cuda(),
              "decode_attn_split_q8: all tensors must be on the GPU");
  if (nsplit == 0) {
    const int64_t blocks = (int64_t)b * nkv * ((nh / nkv + 15) / 16);
    nsplit = (2 * 256 + blocks - 1) / blocks;
    nsplit = std::min<int64_t>(nsplit, (L + 255) / 256);
    nsplit = std::max<int64_t>(std::min<int64_t>(nsplit, 64), 1);
  }
  auto ctx = at::empty({b, nh * d}, qkv.options());
  at::Tensor ws;
  if (nsplit > 1)
    ws = at::empty({b, nh, nsplit, d + 2}, qkv.options().dtype(at::kFloat));
  fs_decode_attn_split_q8(qkv.data_ptr(), kq.data_ptr(),
                          k_scale.data_ptr<float>(), vq.data_ptr(),
                          v_scale.data_ptr<float>(), cos_t.data_ptr<float>(),
                          sin_t.data_ptr<float>(), pos.data_ptr(),
                          (int)pos.numel(),
                          nsplit > 1 ? ws.data_ptr<float>() : nullptr,
                          ctx.data_ptr(), b, nh, nkv, d, L, (float)scale,
                          rope ? 1 : 0, (int)nsplit, cur_stream());
  return ctx;
}

// x bf16 [..., d], d 64 or 128 -> (q int8 [..., d], scale fp32 [...]): the
// row quantisation of the int8 KV cache (decode_attn_q8.hip).
static std::vector<at::Tensor> kv_quantize_int8(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
                  x.is_contiguous() && x.dim() >= 1,
              "kv_quantize_int8: x must be a contiguous bf16 GPU tensor");
  const int d = x.size(-1);
  TORCH_CHECK(d == 64 || d == 128,
              "kv_quantize_int8: last dim must be 64 or 128, got ", d);
  auto q = at::empty(x.sizes(), x.options().dtype(at::kChar));
  auto sc = at::empty(x.sizes().slice(0, x.dim() - 1),
                      x.options().dtype(at::kFloat));
  fs_kv_quantize_int8(x.data_ptr(), q.data_ptr(), sc.data_ptr<float>(),
                      (long)(x.numel() / d), d, cur_stream());
  return {q, sc};
}

// a,b [rows, H] bf16 -> (sum=a+b, y=rmsnorm(sum)*w), inference-only
static std::vector<at::Tensor> add_rms_norm(at::Tensor a, at::Tensor b,
                                            at::Tensor w, double eps) {
  TORCH_CHECK(a.scalar_type() == at::kBFloat16 && a.is_contiguous() &&
              b.is_contiguous() && w.is_contiguous());
  const int H = a.size(-1);
  TORCH_CHECK(H % 8 == 0 && w.numel() == H && b.sizes() == a.sizes());
  const int rows = a.numel() / H;
  auto sum_out = at::empty_like(a);
  auto y = at::empty_like(a);
  fs_add_rms_norm(a.data_ptr(), b.data_ptr(), w.data_ptr(),
                  sum_out.data_ptr(), y.data_ptr(), rows, H, (float)eps,
                  cur_stream());
  return {sum_out, y};
}

// --- block-sparse flash attention ------------------------------------------
// q/k/v [b, h, s, d] bf16 contiguous, d in {64, 96, 128}, s % 16 == 0.
// Tile lists (ops/sparse_flash.py): CSR over (list head, tile) with LH = h
// or 1 (one layout shared by all heads); int32, on q's device.
//   row lists: ptr[LH * ceil(s/128) + 1], idx = 64-key tile index
//   col lists: ptr[LH * ceil(s/64) + 1],  idx = 128-row query tile index
// Everything is checked here, on the host, before anything is launched.
// check_indices additionally copies ptr/idx to the host and verifies the
// CSR structure and every tile index; lists from build_tile_lists are
// verified once when they are built, so the autograd path passes false.
static int check_tile_list(const at::Tensor& ptr, const at::Tensor& idx,
                           const at::Tensor& mask, const at::Tensor& q,
                           int h, int n_lists_per_head, int n_idx_tiles,
                           bool check_indices, const char* name) {
  for (const at::Tensor* t : {&ptr, &idx, &mask}) {
    TORCH_CHECK(t->scalar_type() == at::kInt, "sparse_flash: ", name,
                " lists must be int32");
    TORCH_CHECK(t->device() == q.device(), "sparse_flash: ", name,
                " lists must be on the device of q");
    TORCH_CHECK(t->dim() == 1 && t->is_contiguous(), "sparse_flash: ", name,
                " lists must be 1-D contiguous");
  }
  const int64_t n = ptr.numel() - 1;
  TORCH_CHECK(n == n_lists_per_head || n == (int64_t)h * n_lists_per_head,
              "sparse_flash: ", name, "_ptr has ", ptr.numel(),
              " entries, expected ", n_lists_per_head, "+1 or ",
              (int64_t)h * n_lists_per_head, "+1");
  TORCH_CHECK(idx.numel() == mask.numel(), "sparse_flash: ", name,
              "_idx and ", name, "_mask differ in length");
  if (check_indices) {
    auto p = ptr.cpu();
    auto ix = idx.cpu();
    const int* pp = p.data_ptr<int>();
    const int* ip = ix.data_ptr<int>();
    TORCH_CHECK(pp[0] == 0 && pp[n] == idx.numel(), "sparse_flash: ", name,
                "_ptr does not span ", name, "_idx");
    for (int64_t i = 0; i < n; ++i)
      TORCH_CHECK(pp[i] <= pp[i + 1], "sparse_flash: ", name,
                  "_ptr is not monotone");
    for (int64_t i = 0; i < idx.numel(); ++i)
      TORCH_CHECK(ip[i] >= 0 && ip[i] < n_idx_tiles, "sparse_flash: ", name,
                  "_idx[", i, "] = ", ip[i], " out of range [0, ",
                  n_idx_tiles, ")");
  }
  return n == n_lists_per_head && h != 1 ? 1 : h;
}

static void check_sparse_qkv(const at::Tensor& q, const at::Tensor& k,
                             const at::Tensor& v) {
  TORCH_CHECK(q.is_cuda() && k.is_cuda() && v.is_cuda(),
              "sparse_flash: q/k/v must be on the GPU");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 &&
              k.scalar_type() == at::kBFloat16 &&
              v.scalar_type() == at::kBFloat16, "sparse_flash: bf16 only");
  TORCH_CHECK(q.dim() == 4 && k.sizes() == q.sizes() && v.sizes() == q.sizes(),
              "sparse_flash: q/k/v must be [b, h, s, d] of one shape");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous(),
              "sparse_flash: q/k/v must be contiguous");
  const int64_t d = q.size(3), s = q.size(2);
  TORCH_CHECK(d == 64 || d == 96 || d == 128,
              "sparse_flash: head_dim must be 64, 96 or 128");
  TORCH_CHECK(s >= 16 && s % 16 == 0,
              "sparse_flash: seq_len must be a positive multiple of 16");
  TORCH_CHECK(q.size(0) <= 65535 && q.size(1) <= 65535,
              "sparse_flash: batch and heads are grid dims (<= 65535)");
}

static const unsigned char* checked_key_mask(
    const c10::optional<at::Tensor>& km, const at::Tensor& q) {
  if (!km.has_value()) return nullptr;
  TORCH_CHECK(km->scalar_type() == at::kByte && km->device() == q.device() &&
              km->is_contiguous() && km->dim() == 2 &&
              km->size(0) == q.size(0) && km->size(1) == q.size(2),
              "sparse_flash: key_mask must be contiguous uint8 [b, s] on the "
              "device of q");
  return km->data_ptr<unsigned char>();
}

static std::vector<at::Tensor> sparse_flash_fwd(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor row_ptr,
    at::Tensor row_idx, at::Tensor row_mask,
    c10::optional<at::Tensor> key_mask, double scale, bool causal,
    bool check_indices) {
  check_sparse_qkv(q, k, v);
  const int b = q.size(0), h = q.size(1), s = q.size(2), d = q.size(3);
  const int nqt = (s + 127) / 128, nkt = (s + 63) / 64;
  const int lh = check_tile_list(row_ptr, row_idx, row_mask, q, h, nqt, nkt,
                                 check_indices, "row");
  const unsigned char* kmp = checked_key_mask(key_mask, q);
  auto o = at::empty_like(q);
  auto lse = at::empty({b, h, s}, q.options().dtype(at::kFloat));
  fs_sparse_flash_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                      lse.data_ptr<float>(), row_ptr.data_ptr<int>(),
                      row_idx.data_ptr<int>(), row_mask.data_ptr<int>(), kmp,
                      b, h, s, d, lh, causal ? 1 : 0, (float)scale,
                      cur_stream());
  return {o, lse};
}

static std::vector<at::Tensor> sparse_flash_bwd(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor dout,
    at::Tensor lse, at::Tensor row_ptr, at::Tensor row_idx,
    at::Tensor row_mask, at::Tensor col_ptr, at::Tensor col_idx,
    at::Tensor col_mask, c10::optional<at::Tensor> key_mask, double scale,
    bool causal, bool check_indices) {
  check_sparse_qkv(q, k, v);
  const int b = q.size(0), h = q.size(1), s = q.size(2), d = q.size(3);
  const int nqt = (s + 127) / 128, nkt = (s + 63) / 64;
  TORCH_CHECK(o.sizes() == q.sizes() && o.is_contiguous() &&
              o.scalar_type() == at::kBFloat16 && o.device() == q.device(),
              "sparse_flash_bwd: o must match q");
  TORCH_CHECK(dout.sizes() == q.sizes() &&
              dout.scalar_type() == at::kBFloat16 &&
              dout.device() == q.device(),
              "sparse_flash_bwd: dout must match q");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
              lse.numel() == (int64_t)b * h * s && lse.device() == q.device(),
              "sparse_flash_bwd: lse must be fp32 [b, h, s]");
  const int lh = check_tile_list(row_ptr, row_idx, row_mask, q, h, nqt, nkt,
                                 check_indices, "row");
  const int lhc = check_tile_list(col_ptr, col_idx, col_mask, q, h, nkt, nqt,
                                  check_indices, "col");
  TORCH_CHECK(lh == lhc, "sparse_flash_bwd: row and column lists disagree on "
              "per-head vs shared layout");
  const unsigned char* kmp = checked_key_mask(key_mask, q);
  auto dout_c = dout.contiguous();
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  auto delta = at::empty({b, h, s}, q.options().dtype(at::kFloat));
  fs_sparse_flash_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                      dout_c.data_ptr(), lse.data_ptr<float>(), dq.data_ptr(),
                      dk.data_ptr(), dv.data_ptr(), delta.data_ptr<float>(),
                      row_ptr.data_ptr<int>(), row_idx.data_ptr<int>(),
                      row_mask.data_ptr<int>(), col_ptr.data_ptr<int>(),
                      col_idx.data_ptr<int>(), col_mask.data_ptr<int>(), kmp,
                      b, h, s, d, lh, causal ? 1 : 0, (float)scale,
                      cur_stream());
  return {dq, dk, dv};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("sparse_flash_fwd", &sparse_flash_fwd);
  mod.def("sparse_flash_bwd", &sparse_flash_bwd);
  mod.def("w8_gemv", &w8_gemv);
  mod.def("bf16_gemv", &bf16_gemv);
  mod.def("decode_attn", &decode_attn);
  mod.def("decode_gemm", &decode_gemm, py::arg("w"), py::arg("x"),
          py::arg("scale") = py::none());
  mod.def("decode_gemm_w4", &decode_gemm_w4, py::arg("qweight"),
          py::arg("scales"), py::arg("x"), py::arg("out"),
          py::arg("ksplit") = 0, py::arg("tw") = 0);
  mod.def("decode_attn_split", &decode_attn_split, py::arg("qkv"),
          py::arg("kc"), py::arg("vc"), py::arg("cos"), py::arg("sin"),
          py::arg("pos"), py::arg("scale"), py::arg("rope"),
          py::arg("nsplit") = 0, py::arg("tokens") = 1);
  mod.def("decode_attn_split_q8", &decode_attn_split_q8, py::arg("qkv"),
          py::arg("kq"), py::arg("k_scale"), py::arg("vq"),
          py::arg("v_scale"), py::arg("cos"), py::arg("sin"), py::arg("pos"),
          py::arg("scale"), py::arg("rope"), py::arg("nsplit") = 0);
  mod.def("kv_quantize_int8", &kv_quantize_int8);
  mod.def("add_rms_norm", &add_rms_norm);
  mod.def("flash_attn_fwd", &flash_attn_fwd);
  mod.def("vocab_ce_fwd", [](at::Tensor logits2d, at::Tensor targets,
                             int64_t vstart, int64_t vend) {
    TORCH_CHECK(logits2d.is_contiguous() && logits2d.dim() == 2
                && logits2d.scalar_type() == at::kBFloat16);
    TORCH_CHECK(targets.scalar_type() == at::kLong
                && targets.is_contiguous());
    const long n = logits2d.size(0);
    const int w = logits2d.size(1);
    TORCH_CHECK(w % 8 == 0, "vocab shard must be divisible by 8");
    auto opts = logits2d.options().dtype(at::kFloat);
    auto m = at::empty({n}, opts);
    auto z = at::empty({n}, opts);
    auto pred = at::empty({n}, opts);
    fs_vocab_ce_fwd(logits2d.data_ptr(), targets.data_ptr<long>(),
                    m.data_ptr<float>(), z.data_ptr<float>(),
                    pred.data_ptr<float>(), n, w, (int)vstart, (int)vend,
                    cur_stream());
    return std::vector<at::Tensor>{m, z, pred};
  });
  mod.def("vocab_ce_bwd", [](at::Tensor logits2d, at::Tensor targets,
                             at::Tensor m, at::Tensor z, at::Tensor gout,
                             int64_t vstart, int64_t vend) {
    const long n = logits2d.size(0);
    const int w = logits2d.size(1);
    auto dl = at::empty_like(logits2d);
    fs_vocab_ce_bwd(logits2d.data_ptr(), targets.data_ptr<long>(),
                    m.data_ptr<float>(), z.data_ptr<float>(),
                    gout.contiguous().data_ptr<float>(), dl.data_ptr(), n, w,
                    (int)vstart, (int)vend, cur_stream());
    return dl;
  });
  mod.def("flash_attn_fwd_v3", &flash_attn_fwd_v3, py::arg("q"), py::arg("k"),
          py::arg("v"), py::arg("scale"), py::arg("causal"), py::arg("klens"),
          py::arg("drop_p"), py::arg("seed"), py::arg("kstart") = py::none(),
          py::arg("check_values") = false);
  mod.def("flash_attn_bwd_v3", &flash_attn_bwd_v3, py::arg("q"), py::arg("k"),
          py::arg("v"), py::arg("o"), py::arg("dout"), py::arg("lse"),
          py::arg("scale"), py::arg("causal"), py::arg("klens"),
          py::arg("drop_p"), py::arg("seed"), py::arg("kstart") = py::none(),
          py::arg("qend") = py::none(), py::arg("check_values") = false);
  mod.def("flash_attn_bwd", &flash_attn_bwd);
  mod.def("flash_attn_fwd_v3_strided", &flash_attn_fwd_v3_strided,
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
          py::arg("scale"), py::arg("causal"), py::arg("klens"),
          py::arg("kstart") = py::none(), py::arg("check_values") = false);
  mod.def("flash_attn_bwd_v3_strided", &flash_attn_bwd_v3_strided,
          py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
          py::arg("dout"), py::arg("lse"), py::arg("dq"), py::arg("dk"),
          py::arg("dv"), py::arg("scale"), py::arg("causal"),
          py::arg("klens"), py::arg("kstart") = py::none(),
          py::arg("qend") = py::none(), py::arg("check_values") = false);
  mod.def("flash_v3_block_map", &flash_v3_block_map, py::arg("nx"),
          py::arg("ny"), py::arg("nz"), py::arg("heavy_last"));
  mod.def("rope_inplace", &rope_inplace);
  mod.def("rope_inplace_one", &rope_inplace_one);
  mod.def("rms_norm_fwd", &rms_norm_fwd);
  mod.def("rms_norm_bwd", &rms_norm_bwd);
  mod.def("residual_rms_norm_fwd", &residual_rms_norm_fwd);
  mod.def("residual_rms_norm_bwd", &residual_rms_norm_bwd);
  mod.def("fused_norm_branch", &fused_norm_branch);
  mod.def("layer_norm_fwd", &layer_norm_fwd);
  mod.def("layer_norm_bwd", &layer_norm_bwd);
  mod.def("scaled_masked_softmax_fwd", &scaled_masked_softmax_fwd);
  mod.def("scaled_causal_softmax_fwd", &scaled_causal_softmax_fwd);
  mod.def("scaled_softmax_bwd", &scaled_softmax_bwd);
  mod.def("rope_fwd", &rope_fwd);
  mod.def("rope_bwd", &rope_bwd);
  mod.def("swiglu_fwd", &swiglu_fwd);
  mod.def("swiglu_bwd", &swiglu_bwd);
  mod.def("swiglu_bwd_act", &swiglu_bwd_act, py::arg("gy"),
          py::arg("packed"), py::arg("act_out") = py::none());
  mod.def("bias_gelu_fwd", &bias_gelu_fwd);
  mod.def("bias_gelu_bwd", &bias_gelu_bwd);
  mod.def("fused_adamw", &fused_adamw);
}
