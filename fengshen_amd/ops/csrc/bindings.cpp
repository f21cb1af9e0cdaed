// Torch bindings for fengshen_amd HIP kernels (gfx950).
// Kernels live in kernels.hip / flash_attn.hip as extern "C" launchers taking
// raw pointers + hipStream_t; this file owns all Tensor plumbing.
#include <torch/extension.h>

#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include <string>
#include <vector>

#include "flash_blockmap.h"

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
void fs_decode_attn(const void*, void*, void*, const float*, const float*,
                    const void*, void*, int, int, int, int, int, float, int,
                    hipStream_t);
void fs_w8_gemv(const void*, const float*, const void*, void*, int, int, int,
                hipStream_t);
void fs_vocab_ce_fwd(const void*, const long*, float*, float*, float*,
                     long, int, int, int, hipStream_t);
void fs_vocab_ce_bwd(const void*, const long*, const float*, const float*,
                     const float*, void*, long, int, int, int, hipStream_t);
void fs_flash_attn_fwd_v3(const void*, const void*, const void*, void*,
                          float*, const int*, int, int, int, int, int, float,
                          float, unsigned long long, hipStream_t);
void fs_flash_attn_bwd_v3(const void*, const void*, const void*, const void*,
                          const void*, const float*, void*, void*, void*,
                          float*, const int*, int, int, int, int, int, float,
                          float, unsigned long long, hipStream_t);
void fs_flash_attn_fwd_v3_strided(const void*, const void*, const void*,
                                  void*, float*, const int*, const long*,
                                  const long*, int, int, int, int, int, float,
                                  float, unsigned long long, hipStream_t);
void fs_flash_attn_bwd_v3_strided(const void*, const void*, const void*,
                                  const void*, const void*, const float*,
                                  void*, void*, void*, float*, const int*,
                                  const long*, const long*, const long*,
                                  const long*, int, int, int, int, int, float,
                                  float, unsigned long long, hipStream_t);
void fs_flash_attn_fwd_v3_kstart(const void*, const void*, const void*, void*,
                                 float*, const int*, const long*, const long*,
                                 int, int, int, int, float, hipStream_t);
void fs_flash_attn_bwd_v3_kstart(const void*, const void*, const void*,
                                 const void*, const void*, const float*,
                                 void*, void*, void*, float*, const int*,
                                 const int*, const long*, const long*,
                                 const long*, const long*, int, int, int, int,
                                 float, hipStream_t);
void fs_flash_attn_fwd_v3_gqa(const void*, const void*, const void*, void*,
                              float*, const int*, const long*, const long*,
                              const long*, int, int, int, int, int, float,
                              hipStream_t);
void fs_flash_attn_bwd_v3_gqa(const void*, const void*, const void*,
                              const void*, const void*, const float*, void*,
                              void*, void*, float*, const int*, const int*,
                              const long*, const long*, const long*,
                              const long*, const long*, const long*, int, int,
                              int, int, int, float, hipStream_t);
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
static void check_strided_view(const at::Tensor& t, const char* name, int b,
                               int h, int s, int d) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16, name,
              ": must be a bf16 GPU tensor");
  TORCH_CHECK(t.dim() == 4 && t.size(0) == b && t.size(1) == h &&
                  t.size(2) == s && t.size(3) == d,
              name, ": expected shape [", b, ", ", h, ", ", s, ", ", d, "]");
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
              klens->numel() == b && klens->is_contiguous());
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

// Writes o in place; returns lse [b, h, s] fp32.
static at::Tensor flash_attn_fwd_v3_strided(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, double scale,
    bool causal, c10::optional<at::Tensor> klens,
    c10::optional<at::Tensor> kstart, bool check_values) {
  TORCH_CHECK(q.dim() == 4, "q must be [b, h, s, d]");
  const int b = q.size(0), h = q.size(1), s = q.size(2), d = q.size(3);
  TORCH_CHECK((d == 128 || d == 96 || d == 64) && s % 64 == 0 && s >= 64,
              "flash v3: d in {64, 96, 128}, s a multiple of 64");
  const int h_kv = checked_kv_heads(k, h, causal, 0.0, klens.has_value());
  check_strided_view(q, "q", b, h, s, d);
  check_strided_view(k, "k", b, h_kv, s, d);
  check_strided_view(v, "v", b, h_kv, s, d);
  check_strided_view(o, "o", b, h, s, d);
  if (h_kv == h) check_same_strides(q, k, "q and k");
  check_same_strides(k, v, "k and v");
  if (kstart.has_value())
    check_kstart(*kstart, c10::nullopt, false, q, causal, 0.0,
                 klens.has_value(), check_values);
  const int* klp = checked_klens(klens, causal, b);
  long qs[3], os[3];
  strides3(q, qs);
  strides3(o, os);
  auto lse = at::empty({b, h, s}, q.options().dtype(at::kFloat));
  if (h_kv != h) {
    long kvs[3];
    strides3(k, kvs);
    fs_flash_attn_fwd_v3_gqa(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
        lse.data_ptr<float>(),
        kstart.has_value() ? kstart->data_ptr<int>() : nullptr, qs, kvs, os,
        b, h, h_kv, s, d, (float)scale, cur_stream());
    return lse;
  }
  if (kstart.has_value()) {
    fs_flash_attn_fwd_v3_kstart(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                o.data_ptr(), lse.data_ptr<float>(),
                                kstart->data_ptr<int>(), qs, os, b, h, s, d,
                                (float)scale, cur_stream());
    return lse;
  }
  fs_flash_attn_fwd_v3_strided(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                               o.data_ptr(), lse.data_ptr<float>(), klp, qs,
                               os, b, h, s, d, causal ? 1 : 0, (float)scale,
                               0.f, 0ull, cur_stream());
  return lse;
}

// Writes dq, dk, dv in place.
static void flash_attn_bwd_v3_strided(
    at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor dout,
    at::Tensor lse, at::Tensor dq, at::Tensor dk, at::Tensor dv, double scale,
    bool causal, c10::optional<at::Tensor> klens,
    c10::optional<at::Tensor> kstart, c10::optional<at::Tensor> qend,
    bool check_values) {
  TORCH_CHECK(q.dim() == 4, "q must be [b, h, s, d]");
  const int b = q.size(0), h = q.size(1), s = q.size(2), d = q.size(3);
  TORCH_CHECK((d == 128 || d == 96 || d == 64) && s % 64 == 0 && s >= 64,
              "flash v3: d in {64, 96, 128}, s a multiple of 64");
  const int h_kv = checked_kv_heads(k, h, causal, 0.0, klens.has_value());
  check_strided_view(q, "q", b, h, s, d);
  check_strided_view(k, "k", b, h_kv, s, d);
  check_strided_view(v, "v", b, h_kv, s, d);
  check_strided_view(o, "o", b, h, s, d);
  check_strided_view(dout, "dout", b, h, s, d);
  check_strided_view(dq, "dq", b, h, s, d);
  check_strided_view(dk, "dk", b, h_kv, s, d);
  check_strided_view(dv, "dv", b, h_kv, s, d);
  if (h_kv == h) {
    check_same_strides(q, k, "q and k");
    check_same_strides(dq, dk, "dq and dk");
  }
  check_same_strides(k, v, "k and v");
  check_same_strides(dk, dv, "dk and dv");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat &&
              lse.is_contiguous() && lse.numel() == (int64_t)b * h * s,
              "lse must be contiguous fp32 [b, h, s]");
  if (kstart.has_value())
    check_kstart(*kstart, qend, true, q, causal, 0.0, klens.has_value(),
                 check_values);
  else
    TORCH_CHECK(!qend.has_value(), "flash v3: qend without kstart");
  const int* klp = checked_klens(klens, causal, b);
  long qs[3], os[3], dos[3], gs[3];
  strides3(q, qs);
  strides3(o, os);
  strides3(dout, dos);
  strides3(dq, gs);
  auto delta = at::empty({b, h, s}, q.options().dtype(at::kFloat));
  if (h_kv != h) {
    long kvs[3], gkvs[3];
    strides3(k, kvs);
    strides3(dk, gkvs);
    const bool ks = kstart.has_value();
    fs_flash_attn_bwd_v3_gqa(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
        dout.data_ptr(), lse.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(),
        dv.data_ptr(), delta.data_ptr<float>(),
        ks ? kstart->data_ptr<int>() : nullptr,
        ks ? qend->data_ptr<int>() : nullptr, qs, kvs, os, dos, gs, gkvs, b,
        h, h_kv, s, d, (float)scale, cur_stream());
    return;
  }
  if (kstart.has_value()) {
    fs_flash_attn_bwd_v3_kstart(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
        dout.data_ptr(), lse.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(),
        dv.data_ptr(), delta.data_ptr<float>(), kstart->data_ptr<int>(),
        qend->data_ptr<int>(), qs, os, dos, gs, b, h, s, d, (float)scale,
        cur_stream());
    return;
  }
  fs_flash_attn_bwd_v3_strided(
      q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dout.data_ptr(),
      lse.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
      delta.data_ptr<float>(), klp, qs, os, dos, gs, b, h, s, d,
      causal ? 1 : 0, (float)scale, 0.f, 0ull, cur_stream());
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
  TORCH_CHECK(cos.is_cuda() && sin.is_cuda() &&
              cos.scalar_type() == at::kFloat &&
              sin.scalar_type() == at::kFloat && cos.is_contiguous() &&
              sin.is_contiguous() && cos.dim() == 2 && cos.size(1) == hn &&
              sin.sizes() == cos.sizes(),
              "cos/sin must be contiguous fp32 [S, hn]");
  TORCH_CHECK(offset >= 0 && offset + s <= cos.size(0),
              "rope table too short for offset + s");
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
  TORCH_CHECK(cos.is_cuda() && sin.is_cuda() &&
              cos.scalar_type() == at::kFloat &&
              sin.scalar_type() == at::kFloat && cos.is_contiguous() &&
              sin.is_contiguous() && cos.dim() == 2 && cos.size(1) == hn &&
              sin.sizes() == cos.sizes(),
              "cos/sin must be contiguous fp32 [S, hn]");
  TORCH_CHECK(offset >= 0 && offset + s <= cos.size(0),
              "rope table too short for offset + s");
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
  mod.def("flash_attn_bwd_v3", [](at::Tensor q, at::Tensor k, at::Tensor v,
                                  at::Tensor o, at::Tensor dout,
                                  at::Tensor lse, double scale, bool causal,
                                  c10::optional<at::Tensor> klens,
                                  double drop_p, int64_t seed,
                                  c10::optional<at::Tensor> kstart,
                                  c10::optional<at::Tensor> qend,
                                  bool check_values) {
    const int b = q.size(0), h = q.size(1), s = q.size(2), d = q.size(3);
    TORCH_CHECK((d == 128 || d == 96 || d == 64) && s % 64 == 0);
    const bool gqa =
        checked_kv_heads(k, h, causal, drop_p, klens.has_value()) != h;
    if (kstart.has_value() || gqa) {
      // the kstart and GQA kernels have one (strided) entry; contiguous
      // operands are its special case and get all of its checks
      TORCH_CHECK(drop_p == 0.0, "flash v3: kstart does not support dropout");
      TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
      auto dq = at::empty_like(q);
      auto dk = at::empty_like(k);
      auto dv = at::empty_like(v);
      flash_attn_bwd_v3_strided(q, k, v, o, dout.contiguous(), lse, dq, dk,
                                dv, scale, causal, klens, kstart, qend,
                                check_values);
      return std::vector<at::Tensor>{dq, dk, dv};
    }
    TORCH_CHECK(!qend.has_value(), "flash v3: qend without kstart");
    const int* klp = nullptr;
    if (klens.has_value()) klp = klens->data_ptr<int>();
    auto dq = at::empty_like(q);
    auto dk = at::empty_like(k);
    auto dv = at::empty_like(v);
    auto delta = at::empty({b, h, s}, q.options().dtype(at::kFloat));
    fs_flash_attn_bwd_v3(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                         o.data_ptr(), dout.contiguous().data_ptr(),
                         lse.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(),
                         dv.data_ptr(), delta.data_ptr<float>(), klp, b, h,
                         s, d, causal ? 1 : 0, (float)scale, (float)drop_p,
                         (unsigned long long)seed, cur_stream());
    return std::vector<at::Tensor>{dq, dk, dv};
  }, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("dout"),
     py::arg("lse"), py::arg("scale"), py::arg("causal"), py::arg("klens"),
     py::arg("drop_p"), py::arg("seed"), py::arg("kstart") = py::none(),
     py::arg("qend") = py::none(), py::arg("check_values") = false);
  mod.def("flash_attn_fwd_v3", [](at::Tensor q, at::Tensor k, at::Tensor v,
                                  double scale, bool causal,
                                  c10::optional<at::Tensor> klens,
                                  double drop_p, int64_t seed,
                                  c10::optional<at::Tensor> kstart,
                                  bool check_values) {
    TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
    TORCH_CHECK(q.scalar_type() == at::kBFloat16);
    const int b = q.size(0), h = q.size(1), s = q.size(2), d = q.size(3);
    TORCH_CHECK((d == 128 || d == 96 || d == 64) && s % 64 == 0 && s >= 64);
    TORCH_CHECK(k.size(2) == s, "v3 is self-attention (sq == sk)");
    const bool gqa =
        checked_kv_heads(k, h, causal, drop_p, klens.has_value()) != h;
    if (kstart.has_value() || gqa) {
      TORCH_CHECK(drop_p == 0.0, "flash v3: kstart does not support dropout");
      auto o = at::empty_like(q);
      auto lse = flash_attn_fwd_v3_strided(q, k, v, o, scale, causal, klens,
                                           kstart, check_values);
      return std::vector<at::Tensor>{o, lse};
    }
    const int* klp = nullptr;
    if (klens.has_value()) {
      TORCH_CHECK(klens->scalar_type() == at::kInt
                  && klens->numel() == b && klens->is_contiguous());
      klp = klens->data_ptr<int>();
    }
    auto o = at::empty_like(q);
    auto lse = at::empty({b, h, s}, q.options().dtype(at::kFloat));
    fs_flash_attn_fwd_v3(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                         o.data_ptr(), lse.data_ptr<float>(), klp, b, h, s,
                         d, causal ? 1 : 0, (float)scale, (float)drop_p,
                         (unsigned long long)seed, cur_stream());
    return std::vector<at::Tensor>{o, lse};
  }, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
     py::arg("causal"), py::arg("klens"), py::arg("drop_p"), py::arg("seed"),
     py::arg("kstart") = py::none(), py::arg("check_values") = false);
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
  mod.def("bias_gelu_fwd", &bias_gelu_fwd);
  mod.def("bias_gelu_bwd", &bias_gelu_bwd);
  mod.def("fused_adamw", &fused_adamw);
}
