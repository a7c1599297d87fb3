// Python bindings for the VFA gfx950 HIP kernels (torch extension ABI).
// Kernels live in the sibling .hip TUs behind a C ABI so this (slow,
// torch-header-heavy) TU rarely recompiles.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <mutex>
#include <unordered_map>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

extern "C" {
void vfa_quick_gelu(const void*, void*, long long, int, hipStream_t);
void vfa_gelu_tanh(const void*, void*, long long, int, hipStream_t);
void vfa_layer_norm(const void*, const void*, const void*, void*, long long,
                    int, float, int, hipStream_t);
void vfa_bilinear_warp(const void*, const void*, void*, int, int, int, int,
                       int, hipStream_t);
void vfa_bilinear_warp_nhwc(const void*, const void*, void*, int, int, int,
                            int, long long, long long, long long, long long,
                            float, hipStream_t);
void vfa_pwc_correlation_nhwc(const void*, const void*, void*, int, int, int,
                              int, int, int, hipStream_t);
long long vfa_tconv_lds_bytes(int, int);
void vfa_tconv_pform(const void*, const void*, const void*, void*, void*, int,
                     int, int, int, int, int, int, hipStream_t);
void vfa_tconv_direct(const void*, const void*, const void*, void*, int, int,
                      int, int, long long, long long, long long, long long,
                      int, int, hipStream_t);
void vfa_grid_sample(const void*, const void*, void*, long long, int, int,
                     int, int, int, int, hipStream_t);
void vfa_corr_repack(const void*, void*, int, int, int, int, int,
                     hipStream_t);
void vfa_pwc_correlation(const void*, const void*, const void*, void*, int,
                         int, int, int, int, int, int, hipStream_t);
void vfa_mhsa_small(const void*, const void*, const void*, void*, int, int,
                    int, float, int, hipStream_t);
void vfa_flash_qkv(const void*, void*, int, int, int, float, hipStream_t);
void vfa_mfma_gemm16(const void*, const void*, void*, hipStream_t);
void vfa_layer_norm_residual(const void*, const void*, const void*,
                             const void*, void*, void*, long long, int,
                             float, int, hipStream_t);
void vfa_u8_chw_norm(const void*, void*, long long, int, int, const float*,
                     const float*, int, hipStream_t);
void vfa_corr_lookup(const void*, const void*, const void*, const void*,
                     const void*, void*, int, int, int, int, int, int, int,
                     int, int, long long, int, int, int, int, hipStream_t);
void vfa_convex_upsample(const void*, const void*, void*, int, int, int, int,
                         int, hipStream_t);
void vfa_gru_zr(const void*, const void*, void*, void*, int, int, int,
                long long, int, int, hipStream_t);
void vfa_gru_out(const void*, const void*, void*, int, int, int, long long,
                 int, int, hipStream_t);
void vfa_instance_norm2d(const void*, void*, int, int, int, float, int, int,
                         int, hipStream_t);
void vfa_maxpool3d_same(const void*, void*, long long, int, int, int, int,
                        int, int, int, int, int, int, int, int, int, int,
                        int, int, hipStream_t);
void vfa_maxpool2d_same(const void*, void*, long long, int, int, int, int,
                        int, int, int, int, int, int, int, int, int,
                        hipStream_t);
void vfa_linear_res_stats(const void*, const void*, const void*, const void*,
                          void*, void*, int, int, int, hipStream_t);
void vfa_linear_ln_act(const void*, const void*, int, const void*,
                       const void*, const void*, void*, int, int, int, float,
                       int, hipStream_t);
void vfa_linear_act(const void*, const void*, const void*, const void*,
                    void*, int, int, int, int, hipStream_t);
void vfa_temporal_merge(const void*, void*, int, int, int, int, int, int,
                        int, long long, int, int, hipStream_t);
void vfa_conv2d_nhwc(const void*, const void*, const void*, const void*,
                     const void*, void*, int, int, int, int, int, int, int,
                     int, int, int, int, int, int, int, int, int, int, int,
                     hipStream_t);
void vfa_conv2d_pick_tile(int, int, int*, int*);
void vfa_pad2d_nhwc(const void*, void*, int, int, int, int, int, int, int,
                    int, int, hipStream_t);
void vfa_avgpool2d_nhwc(const void*, void*, long long, int, int, int, int,
                        int, int, hipStream_t);
void vfa_attnpool_tokens(const void*, const void*, void*, long long, int, int,
                         hipStream_t);
void vfa_attention_pool_d64(const void*, const void*, void*, long long, int,
                            int, float, hipStream_t);
void vfa_clip_embed_ln(const void*, const void*, const void*, const void*,
                       const void*, void*, long long, int, int, float, int,
                       hipStream_t);
}

namespace {

int dtype_tag(const torch::Tensor& t) {
  switch (t.scalar_type()) {
    case torch::kFloat32: return 0;
    case torch::kBFloat16: return 1;
    case torch::kFloat16: return 2;
    default:
      TORCH_CHECK(false, "unsupported dtype ", t.scalar_type());
  }
}

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

torch::Tensor quick_gelu(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  auto out = torch::empty_like(x);
  vfa_quick_gelu(x.data_ptr(), out.data_ptr(), x.numel(), dtype_tag(x),
                 current_stream());
  return out;
}

torch::Tensor gelu_tanh(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  auto out = torch::empty_like(x);
  vfa_gelu_tanh(x.data_ptr(), out.data_ptr(), x.numel(), dtype_tag(x),
                current_stream());
  return out;
}

torch::Tensor layer_norm(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                         double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  const int d = (int)x.size(-1);
  TORCH_CHECK(w.numel() == d && b.numel() == d, "affine shape mismatch");
  auto wc = w.contiguous().to(x.scalar_type());
  auto bc = b.contiguous().to(x.scalar_type());
  auto out = torch::empty_like(x);
  vfa_layer_norm(x.data_ptr(), wc.data_ptr(), bc.data_ptr(), out.data_ptr(),
                 x.numel() / d, d, (float)eps, dtype_tag(x), current_stream());
  return out;
}

// (T, P, W) patch embeddings + cls (W) + pos (P+1, W) -> ln_pre'd tokens
// (T, P+1, W); see clip_embed_ln_kernel
torch::Tensor clip_embed_ln(torch::Tensor pe, torch::Tensor cls,
                            torch::Tensor pos, torch::Tensor w,
                            torch::Tensor b, double eps) {
  TORCH_CHECK(pe.is_cuda() && pe.is_contiguous() && pe.dim() == 3,
              "clip_embed_ln: pe must be a contiguous (T, P, W) GPU tensor");
  const long long t = pe.size(0);
  const int p = (int)pe.size(1), d = (int)pe.size(2);
  TORCH_CHECK(d % 8 == 0, "clip_embed_ln: W % 8 == 0 required");
  TORCH_CHECK(cls.numel() == d && w.numel() == d && b.numel() == d &&
                  pos.dim() == 2 && pos.size(0) == p + 1 && pos.size(1) == d,
              "clip_embed_ln: shape mismatch");
  auto cc = cls.contiguous().to(pe.scalar_type());
  auto pc = pos.contiguous().to(pe.scalar_type());
  auto wc = w.contiguous().to(pe.scalar_type());
  auto bc = b.contiguous().to(pe.scalar_type());
  auto out = torch::empty({(long)t, p + 1, d}, pe.options());
  vfa_clip_embed_ln(pe.data_ptr(), cc.data_ptr(), pc.data_ptr(),
                    wc.data_ptr(), bc.data_ptr(), out.data_ptr(),
                    t * (p + 1), p, d, (float)eps, dtype_tag(pe),
                    current_stream());
  return out;
}

torch::Tensor bilinear_warp(torch::Tensor x, torch::Tensor flow) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && flow.is_contiguous());
  TORCH_CHECK(x.dim() == 4 && flow.dim() == 4 && flow.size(1) == 2);
  auto flow_c = flow.to(x.scalar_type()).contiguous();
  auto out = torch::empty_like(x);
  vfa_bilinear_warp(x.data_ptr(), flow_c.data_ptr(), out.data_ptr(),
                    (int)x.size(0), (int)x.size(1), (int)x.size(2),
                    (int)x.size(3), dtype_tag(x), current_stream());
  return out;
}

bool cl_only(const torch::Tensor& t) {
  return t.dim() == 4 &&
         t.is_contiguous(torch::MemoryFormat::ChannelsLast) &&
         !t.is_contiguous();
}

// x channels_last bf16 (C % 8 == 0); flow bf16 (B, 2, H, W) of ANY strides,
// read in place; sample point (x + scale*fx, y + scale*fy); channels_last
// result
torch::Tensor bilinear_warp_nhwc(torch::Tensor x, torch::Tensor flow,
                                 double scale) {
  TORCH_CHECK(x.is_cuda() && cl_only(x) &&
                  x.scalar_type() == torch::kBFloat16 && x.size(1) % 8 == 0,
              "bilinear_warp_nhwc: x must be channels_last bf16, C % 8 == 0");
  TORCH_CHECK(flow.is_cuda() && flow.dim() == 4 && flow.size(1) == 2 &&
                  flow.scalar_type() == torch::kBFloat16 &&
                  flow.size(0) == x.size(0) && flow.size(2) == x.size(2) &&
                  flow.size(3) == x.size(3),
              "bilinear_warp_nhwc: flow must be bf16 (B, 2, H, W)");
  auto out = torch::empty_like(x);   // preserves channels_last
  TORCH_CHECK(cl_only(out) || out.numel() == 0);
  if (x.numel() == 0) return out;
  vfa_bilinear_warp_nhwc(x.data_ptr(), flow.data_ptr(), out.data_ptr(),
                         (int)x.size(0), (int)x.size(1), (int)x.size(2),
                         (int)x.size(3), flow.stride(0), flow.stride(1),
                         flow.stride(2), flow.stride(3), (float)scale,
                         current_stream());
  return out;
}

// f1, f2 channels_last bf16, read unpadded and in place.  out_buf as in
// pwc_correlation; without it the result is a channels_last bf16
// (B, 81, H, W) tensor
torch::Tensor pwc_correlation_nhwc(torch::Tensor f1, torch::Tensor f2,
                                   c10::optional<torch::Tensor> out_buf,
                                   int64_t out_off, bool leaky) {
  TORCH_CHECK(f1.is_cuda() && f2.is_cuda() && cl_only(f1) && cl_only(f2) &&
                  f1.scalar_type() == torch::kBFloat16 &&
                  f2.scalar_type() == torch::kBFloat16,
              "pwc_correlation_nhwc: inputs must be channels_last bf16");
  TORCH_CHECK(f1.sizes() == f2.sizes());
  TORCH_CHECK(f1.size(1) <= 256,
              "corr_wave registers cover C<=256 (PWC max is 196)");
  const int b = (int)f1.size(0), c = (int)f1.size(1);
  const int h = (int)f1.size(2), w = (int)f1.size(3);
  torch::Tensor out;
  if (out_buf.has_value()) {
    out = *out_buf;
    TORCH_CHECK(out.is_cuda() && out.dim() == 4 &&
                out.is_contiguous(torch::MemoryFormat::ChannelsLast) &&
                out.scalar_type() == torch::kBFloat16 && out.size(0) == b &&
                out.size(2) == h && out.size(3) == w && out_off >= 0 &&
                out_off + 81 <= out.size(1),
                "out buffer must be CL bf16 (B, >=off+81, H, W)");
  } else {
    out_off = 0;
    out = torch::empty({b, h, w, 81}, f1.options()).permute({0, 3, 1, 2});
  }
  vfa_pwc_correlation_nhwc(f1.data_ptr(), f2.data_ptr(),
                           static_cast<char*>(out.data_ptr()) + out_off * 2,
                           b, c, h, w, (int)out.size(1), leaky ? 1 : 0,
                           current_stream());
  return out;
}

torch::Tensor grid_sample_bilinear(torch::Tensor x, torch::Tensor coords) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous());
  TORCH_CHECK(coords.dim() == 4 && coords.size(-1) == 2);
  TORCH_CHECK(coords.size(0) == x.size(0));
  auto cc = coords.to(x.scalar_type()).contiguous();
  const long long n = x.size(0);
  const int c = (int)x.size(1), h = (int)x.size(2), w = (int)x.size(3);
  const int ho = (int)coords.size(1), wo = (int)coords.size(2);
  auto out = torch::empty({(long)n, c, ho, wo}, x.options());
  vfa_grid_sample(x.data_ptr(), cc.data_ptr(), out.data_ptr(), n, c, h, w, ho,
                  wo, dtype_tag(x), current_stream());
  return out;
}

torch::Tensor pwc_correlation(torch::Tensor f1, torch::Tensor f2,
                              int64_t max_disp,
                              c10::optional<torch::Tensor> out_buf,
                              int64_t out_off, bool leaky) {
  // out_buf: a (B, >= out_off + 81, H, W) channels_last bf16 buffer; the
  // kernels write the cost volume (LeakyReLU(0.1) of it when leaky) into
  // its channels [out_off, out_off + 81) and nothing else
  TORCH_CHECK(f1.is_cuda() && f1.is_contiguous() && f2.is_contiguous());
  TORCH_CHECK(max_disp == 4, "kernel is specialized for max_disp=4");
  TORCH_CHECK(f1.sizes() == f2.sizes());
  TORCH_CHECK(f1.size(1) <= 256,
              "corr_wave registers cover C<=256 (PWC max is 196)");
  const int b = (int)f1.size(0), c = (int)f1.size(1);
  const int h = (int)f1.size(2), w = (int)f1.size(3);
  auto opts = f1.options();
  auto f1p = torch::empty({b, h + 8, w + 8, c}, opts);
  auto f2p = torch::empty({b, h + 8, w + 8, c}, opts);
  const int tag = dtype_tag(f1);
  auto stream = current_stream();
  // tiled path (c<=64) reads f1 as NCHW directly; wave path needs both packed
  if (c > 64) vfa_corr_repack(f1.data_ptr(), f1p.data_ptr(), b, c, h, w, tag, stream);
  vfa_corr_repack(f2.data_ptr(), f2p.data_ptr(), b, c, h, w, tag, stream);
  if (out_buf.has_value()) {
    auto out = *out_buf;
    TORCH_CHECK(out.is_cuda() && out.dim() == 4 &&
                out.is_contiguous(torch::MemoryFormat::ChannelsLast) &&
                out.scalar_type() == torch::kBFloat16 && out.size(0) == b &&
                out.size(2) == h && out.size(3) == w && out_off >= 0 &&
                out_off + 81 <= out.size(1),
                "out buffer must be CL bf16 (B, >=off+81, H, W)");
    vfa_pwc_correlation(f1.data_ptr(), f1p.data_ptr(), f2p.data_ptr(),
                        static_cast<char*>(out.data_ptr()) + out_off * 2, b,
                        c, h, w, tag, (int)out.size(1), leaky ? 1 : 0,
                        stream);
    return out;
  }
  auto out = torch::empty({b, 81, h, w}, opts.dtype(torch::kFloat32));
  vfa_pwc_correlation(f1.data_ptr(), f1p.data_ptr(), f2p.data_ptr(),
                      out.data_ptr(), b, c, h, w, tag, 0, leaky ? 1 : 0,
                      stream);
  return out.to(f1.scalar_type());
}

torch::Tensor mhsa(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                   double scale) {
  // (B, H, N, D) each, N<=64, D<=128
  TORCH_CHECK(q.is_cuda() && q.is_contiguous() && k.is_contiguous() &&
              v.is_contiguous());
  TORCH_CHECK(q.dim() == 4);
  const int n = (int)q.size(2), d = (int)q.size(3);
  TORCH_CHECK(n <= 64 && d <= 128, "mhsa kernel covers N<=64, D<=128");
  const int bh = (int)(q.size(0) * q.size(1));
  auto out = torch::empty_like(q);
  vfa_mhsa_small(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), bh,
                 n, d, (float)scale, dtype_tag(q), current_stream());
  return out;
}

std::vector<torch::Tensor> layer_norm_residual(torch::Tensor x,
                                               torch::Tensor res,
                                               torch::Tensor w,
                                               torch::Tensor b, double eps) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && res.is_contiguous());
  TORCH_CHECK(x.sizes() == res.sizes());
  const int d = (int)x.size(-1);
  auto wc = w.contiguous().to(x.scalar_type());
  auto bc = b.contiguous().to(x.scalar_type());
  auto y = torch::empty_like(x);
  auto s = torch::empty_like(x);
  vfa_layer_norm_residual(x.data_ptr(), res.data_ptr(), wc.data_ptr(),
                          bc.data_ptr(), y.data_ptr(), s.data_ptr(),
                          x.numel() / d, d, (float)eps, dtype_tag(x),
                          current_stream());
  return {y, s};
}

torch::Tensor u8_chw_norm(torch::Tensor frames, std::vector<double> mean,
                          std::vector<double> std_, bool bf16) {
  TORCH_CHECK(frames.is_cuda() && frames.is_contiguous());
  TORCH_CHECK(frames.scalar_type() == torch::kUInt8);
  TORCH_CHECK(frames.dim() == 4 && frames.size(3) == 3, "(T,H,W,3) expected");
  const long long t = frames.size(0);
  const int h = (int)frames.size(1), w = (int)frames.size(2);
  TORCH_CHECK((h * w) % 4 == 0);
  float m[3] = {(float)mean[0], (float)mean[1], (float)mean[2]};
  float s[3] = {(float)std_[0], (float)std_[1], (float)std_[2]};
  auto out = torch::empty({(long)t, 3, h, w},
                          frames.options().dtype(bf16 ? torch::kBFloat16
                                                      : torch::kFloat32));
  vfa_u8_chw_norm(frames.data_ptr(), out.data_ptr(), t, h, w, m, s,
                  bf16 ? 1 : 0, current_stream());
  return out;
}

torch::Tensor flash_qkv(torch::Tensor qkv, double scale) {
  // qkv: (B, N, 3, H, D) bf16 contiguous, D == 64 -> out (B, N, H*D)
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 5);
  TORCH_CHECK(qkv.size(2) == 3 && qkv.size(4) == 64,
              "flash_qkv covers head_dim 64");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16);
  const int b = (int)qkv.size(0), n = (int)qkv.size(1);
  const int h = (int)qkv.size(3);
  auto out = torch::empty({b, n, h * 64L}, qkv.options());
  vfa_flash_qkv(qkv.data_ptr(), out.data_ptr(), b, n, h, (float)scale,
                current_stream());
  return out;
}

torch::Tensor mfma_gemm16(torch::Tensor a, torch::Tensor b) {
  TORCH_CHECK(a.is_cuda() && a.is_contiguous() && b.is_contiguous());
  TORCH_CHECK(a.sizes() == torch::IntArrayRef({16, 32}) &&
              b.sizes() == torch::IntArrayRef({32, 16}));
  auto af = a.to(torch::kFloat32), bf = b.to(torch::kFloat32);
  auto d = torch::empty({16, 16}, af.options());
  vfa_mfma_gemm16(af.data_ptr(), bf.data_ptr(), d.data_ptr(),
                  current_stream());
  return d;
}

torch::Tensor corr_lookup(std::vector<torch::Tensor> pyramid,
                          torch::Tensor coords, bool nhwc,
                          torch::ScalarType out_dtype, bool force_gmem) {
  // pyramid: up to 4 levels of (N, 1, h_l, w_l) fp32, N = B*H*W; coords
  // (B, 2, H, W) fp32 pixel units at level 0.  Returns (B, L*81, H, W)
  // (contiguous, or channels_last when nhwc) in out_dtype.
  const int levels = (int)pyramid.size();
  TORCH_CHECK(levels >= 1 && levels <= 4, "1..4 pyramid levels");
  TORCH_CHECK(coords.is_cuda() && coords.dim() == 4 && coords.size(1) == 2);
  auto cc = coords.to(torch::kFloat32).contiguous();
  const long long b = coords.size(0);
  const int h = (int)coords.size(2), w = (int)coords.size(3);
  const long long npix = b * h * w;
  int hs[4] = {1, 1, 1, 1}, ws[4] = {1, 1, 1, 1};
  const void* ptrs[4] = {nullptr, nullptr, nullptr, nullptr};
  long long lds_floats = 0;
  for (int l = 0; l < levels; ++l) {
    auto& t = pyramid[l];
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                t.scalar_type() == torch::kFloat32);
    TORCH_CHECK(t.size(0) == npix && t.size(1) == 1, "plane-per-pixel");
    hs[l] = (int)t.size(2);
    ws[l] = (int)t.size(3);
    ptrs[l] = t.data_ptr();
    lds_floats += hs[l] * ws[l];
  }
  for (int l = levels; l < 4; ++l) ptrs[l] = ptrs[levels - 1];
  const int ctot = levels * 81;
  auto opts = coords.options().dtype(out_dtype);
  torch::Tensor out;
  if (nhwc) {
    out = torch::empty({b, h, w, ctot}, opts)
              .permute({0, 3, 1, 2});  // memory is NHWC; view as NCHW
  } else {
    out = torch::empty({b, ctot, h, w}, opts);
  }
  int tag = out_dtype == torch::kFloat32 ? 0
            : out_dtype == torch::kBFloat16 ? 1 : 2;
  vfa_corr_lookup(ptrs[0], ptrs[1], ptrs[2], ptrs[3], cc.data_ptr(),
                  out.data_ptr(), levels, hs[0], ws[0], hs[1], ws[1], hs[2],
                  ws[2], hs[3], ws[3], npix, h * w,
                  (int)((lds_floats <= 16384 && !force_gmem) ? lds_floats : 0),
                  nhwc ? 1 : 0, tag, current_stream());
  return out;
}

static bool cl_contig(const torch::Tensor& t) {
  return t.is_contiguous(torch::MemoryFormat::ChannelsLast);
}

torch::Tensor convex_upsample(torch::Tensor flow, torch::Tensor mask,
                              bool nhwc) {
  TORCH_CHECK(flow.is_cuda() && flow.dim() == 4 && flow.size(1) == 2);
  TORCH_CHECK(mask.dim() == 4 && mask.size(1) == 576);
  TORCH_CHECK(mask.scalar_type() == flow.scalar_type());
  if (nhwc) {
    TORCH_CHECK(cl_contig(flow) && cl_contig(mask), "channels_last expected");
  } else {
    TORCH_CHECK(flow.is_contiguous() && mask.is_contiguous());
  }
  const int b = (int)flow.size(0), h = (int)flow.size(2),
            w = (int)flow.size(3);
  auto out = torch::empty({b, 2, 8 * h, 8 * w}, flow.options());
  vfa_convex_upsample(flow.data_ptr(), mask.data_ptr(), out.data_ptr(), b, h,
                      w, nhwc ? 1 : 0, dtype_tag(flow), current_stream());
  return out;
}

torch::Tensor gru_zr(torch::Tensor zr, torch::Tensor hx, torch::Tensor rhx,
                     bool nhwc) {
  // zr (B,2C,h,w) conv out; hx/rhx (B,C+X,h,w) persistent buffers.
  // Writes r*sigmoid into rhx[:, :C]; returns z (B,C,h,w).
  const int b = (int)zr.size(0), c2 = (int)zr.size(1);
  const int c = c2 / 2, ctot = (int)hx.size(1);
  const long long hw = (long long)zr.size(2) * zr.size(3);
  if (nhwc) {
    TORCH_CHECK(cl_contig(zr) && cl_contig(hx) && cl_contig(rhx));
  } else {
    TORCH_CHECK(zr.is_contiguous() && hx.is_contiguous() &&
                rhx.is_contiguous());
  }
  auto z = nhwc ? torch::empty({b, (int)zr.size(2), (int)zr.size(3), c},
                               zr.options()).permute({0, 3, 1, 2})
                : torch::empty({b, c, (int)zr.size(2), (int)zr.size(3)},
                               zr.options());
  vfa_gru_zr(zr.data_ptr(), hx.data_ptr(), rhx.data_ptr(), z.data_ptr(), b,
             c, ctot - c, hw, nhwc ? 1 : 0, dtype_tag(zr), current_stream());
  return z;
}

void gru_out(torch::Tensor q, torch::Tensor z, torch::Tensor hx, bool nhwc) {
  const int b = (int)q.size(0), c = (int)q.size(1), ctot = (int)hx.size(1);
  const long long hw = (long long)q.size(2) * q.size(3);
  if (nhwc) {
    TORCH_CHECK(cl_contig(q) && cl_contig(hx));
  } else {
    TORCH_CHECK(q.is_contiguous() && hx.is_contiguous());
  }
  vfa_gru_out(q.data_ptr(), z.data_ptr(), hx.data_ptr(), b, c, ctot - c, hw,
              nhwc ? 1 : 0, dtype_tag(q), current_stream());
}

torch::Tensor instance_norm2d(torch::Tensor x, double eps, bool relu,
                              bool nhwc) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4);
  if (nhwc) {
    TORCH_CHECK(cl_contig(x), "channels_last expected");
  } else {
    TORCH_CHECK(x.is_contiguous());
  }
  auto out = torch::empty_like(x);
  vfa_instance_norm2d(x.data_ptr(), out.data_ptr(), (int)x.size(0),
                      (int)x.size(1), (int)(x.size(2) * x.size(3)),
                      (float)eps, relu ? 1 : 0, nhwc ? 1 : 0, dtype_tag(x),
                      current_stream());
  return out;
}

torch::Tensor maxpool3d_same(torch::Tensor x, std::vector<int64_t> kernel,
                             std::vector<int64_t> stride,
                             std::vector<int64_t> pad_front,
                             std::vector<int64_t> out_sz) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 5);
  const long long bc = x.size(0) * x.size(1);
  auto out = torch::empty({x.size(0), x.size(1), out_sz[0], out_sz[1],
                           out_sz[2]}, x.options());
  vfa_maxpool3d_same(x.data_ptr(), out.data_ptr(), bc, (int)x.size(2),
                     (int)x.size(3), (int)x.size(4), (int)out_sz[0],
                     (int)out_sz[1], (int)out_sz[2], (int)kernel[0],
                     (int)kernel[1], (int)kernel[2], (int)stride[0],
                     (int)stride[1], (int)stride[2], (int)pad_front[0],
                     (int)pad_front[1], (int)pad_front[2], dtype_tag(x),
                     current_stream());
  return out;
}

torch::Tensor maxpool2d_same(torch::Tensor x, std::vector<int64_t> kernel,
                             std::vector<int64_t> stride,
                             std::vector<int64_t> pad_front,
                             std::vector<int64_t> out_sz, bool nhwc) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4);
  if (nhwc) {
    TORCH_CHECK(cl_contig(x), "channels_last expected");
  } else {
    TORCH_CHECK(x.is_contiguous());
  }
  auto out = nhwc
      ? torch::empty({x.size(0), out_sz[0], out_sz[1], x.size(1)},
                     x.options()).permute({0, 3, 1, 2})
      : torch::empty({x.size(0), x.size(1), out_sz[0], out_sz[1]},
                     x.options());
  vfa_maxpool2d_same(x.data_ptr(), out.data_ptr(), x.size(0),
                     (int)x.size(1), (int)x.size(2), (int)x.size(3),
                     (int)out_sz[0], (int)out_sz[1], (int)kernel[0],
                     (int)kernel[1], (int)stride[0], (int)stride[1],
                     (int)pad_front[0], (int)pad_front[1], nhwc ? 1 : 0,
                     dtype_tag(x), current_stream());
  return out;
}

torch::Tensor linear_act(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> bias,
                         c10::optional<torch::Tensor> res, int64_t act) {
  // x (M, K) bf16, w (N, K) bf16 (torch Linear layout) -> act(x@w^T+b)
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous());
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              w.scalar_type() == torch::kBFloat16);
  const int m = (int)x.size(0), kk = (int)x.size(1), n = (int)w.size(0);
  // ragged M/N/K handled by the guarded staging path; K%8 keeps the
  // 16-B row segments aligned
  TORCH_CHECK(w.size(1) == kk && kk % 8 == 0, "K%8==0 required");
  TORCH_CHECK(act >= 0 && act <= 4, "linear_act: unknown activation id ",
              act);
  const void* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    bc = bias->contiguous().to(torch::kBFloat16);
    TORCH_CHECK(bc.numel() == n);
    bptr = bc.data_ptr();
  }
  const void* rptr = nullptr;
  if (res.has_value()) {
    TORCH_CHECK(res->is_contiguous() &&
                res->scalar_type() == torch::kBFloat16 &&
                res->numel() == (long long)m * n,
                "residual must be (M, N) bf16 contiguous");
    rptr = res->data_ptr();
  }
  auto out = torch::empty({m, n}, x.options());
  vfa_linear_act(x.data_ptr(), w.data_ptr(), bptr, rptr, out.data_ptr(), m,
                 n, kk, (int)act, current_stream());
  return out;
}

// the fused LayerNorm-fold epilogues exist for full 256^2 tiles only
static void check_full_tiles(const char* op, int m, int n, int k) {
  TORCH_CHECK(m > 0 && m % 256 == 0 && n % 256 == 0 && k % 64 == 0, op,
              ": needs M % 256 == 0, N % 256 == 0, K % 64 == 0, got M=", m,
              " N=", n, " K=", k);
}

std::vector<torch::Tensor> linear_res_stats(torch::Tensor x, torch::Tensor w,
                                            c10::optional<torch::Tensor> bias,
                                            torch::Tensor res) {
  // s = x@w^T + b + res (bf16) and stats (M, N/256, 2) f32: per row and
  // 256-column group the (mean, M2) of the rounded s
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous());
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              w.scalar_type() == torch::kBFloat16);
  const int m = (int)x.size(0), kk = (int)x.size(1), n = (int)w.size(0);
  TORCH_CHECK(w.size(1) == kk);
  check_full_tiles("linear_res_stats", m, n, kk);
  const void* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    bc = bias->contiguous().to(torch::kBFloat16);
    TORCH_CHECK(bc.numel() == n);
    bptr = bc.data_ptr();
  }
  TORCH_CHECK(res.is_cuda() && res.is_contiguous() &&
              res.scalar_type() == torch::kBFloat16 &&
              res.numel() == (long long)m * n,
              "residual must be (M, N) bf16 contiguous");
  auto out = torch::empty({m, n}, x.options());
  auto stats = torch::empty({m, n / 256, 2},
                            x.options().dtype(torch::kFloat32));
  vfa_linear_res_stats(x.data_ptr(), w.data_ptr(), bptr, res.data_ptr(),
                       out.data_ptr(), stats.data_ptr(), m, n, kk,
                       current_stream());
  return {out, stats};
}

torch::Tensor linear_ln_act(torch::Tensor x, torch::Tensor stats,
                            torch::Tensor w, torch::Tensor ln_c,
                            torch::Tensor ln_b, double eps, int64_t act) {
  // act(rstd * (x@w^T - mean * ln_c) + ln_b): x un-normalised rows, w / ln_c
  // / ln_b the LayerNorm-folded linear layer, stats (M, T, 2) the (mean, M2)
  // of T equal-width column groups of each row of x
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous());
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              w.scalar_type() == torch::kBFloat16);
  const int m = (int)x.size(0), kk = (int)x.size(1), n = (int)w.size(0);
  TORCH_CHECK(w.size(1) == kk);
  check_full_tiles("linear_ln_act", m, n, kk);
  TORCH_CHECK(act >= 0 && act <= 4, "linear_ln_act: unknown activation id ",
              act);
  TORCH_CHECK(stats.is_cuda() && stats.is_contiguous() &&
              stats.scalar_type() == torch::kFloat32 && stats.dim() == 3 &&
              stats.size(0) == m && stats.size(2) == 2 &&
              stats.size(1) >= 1 && kk % stats.size(1) == 0,
              "stats must be (M, T, 2) f32 with K % T == 0");
  for (const auto* v : {&ln_c, &ln_b})
    TORCH_CHECK(v->is_cuda() && v->is_contiguous() &&
                v->scalar_type() == torch::kFloat32 && v->numel() == n,
                "ln_c / ln_b must be (N) f32");
  auto out = torch::empty({m, n}, x.options());
  vfa_linear_ln_act(x.data_ptr(), stats.data_ptr(), (int)stats.size(1),
                    w.data_ptr(), ln_c.data_ptr(), ln_b.data_ptr(),
                    out.data_ptr(), m, n, kk, (float)eps, (int)act,
                    current_stream());
  return out;
}

torch::Tensor conv2d_nhwc(torch::Tensor x, torch::Tensor w,
                          c10::optional<torch::Tensor> bias,
                          c10::optional<torch::Tensor> res,
                          int64_t stride_h, int64_t stride_w,
                          int64_t pt, int64_t pb, int64_t pl, int64_t pr,
                          int64_t act,
                          c10::optional<torch::Tensor> out_buf,
                          int64_t out_off, int64_t dil_h, int64_t dil_w,
                          int64_t in_off, int64_t in_ch) {
  // x (B, C, H, W) channels_last bf16; w (K, C, KH, KW) channels_last bf16
  // (physical (K, KH, KW, C) = the (N, Kr) B-operand); out (B, K, OH, OW)
  // channels_last.  Implicit-GEMM MFMA kernel; input pre-padded by the
  // pad2d kernel when C % 8 != 0.
  // in_ch > 0: x is a wider buffer and the conv reads its channels
  // [in_off, in_off + in_ch) in place (pixel stride ldx = x.size(1)).
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && cl_contig(x),
              "x must be channels_last");
  TORCH_CHECK(w.dim() == 4 && cl_contig(w), "w must be channels_last");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              w.scalar_type() == torch::kBFloat16);
  const bool slice = in_ch > 0;
  const int xc = (int)x.size(1);
  if (slice) {
    // each lane's 16-B load must stay aligned and inside one tap
    TORCH_CHECK(in_off >= 0 && in_off % 8 == 0 && in_ch % 8 == 0 &&
                xc % 8 == 0 && in_off + in_ch <= xc,
                "slice input needs in_off, in_ch and the buffer width to be "
                "multiples of 8 and the slice inside the buffer");
  } else {
    TORCH_CHECK(in_off == 0 && in_ch == 0, "in_off needs in_ch > 0");
  }
  TORCH_CHECK(dil_h >= 1 && dil_w >= 1 && stride_h >= 1 && stride_w >= 1);
  const int b = (int)x.size(0), c = slice ? (int)in_ch : xc;
  const int h = (int)x.size(2), ww = (int)x.size(3);
  const int kout = (int)w.size(0), kh = (int)w.size(2), kw = (int)w.size(3);
  // C % 8 != 0 (stems, the RAFT corr input): the pad pass widens the
  // channel dim with zeros; the weight must arrive already zero-padded to
  // the same c8 (conv2d_mod caches that)
  const int c8 = (c + 7) / 8 * 8;
  TORCH_CHECK(w.size(1) == c8, "weight C must be input C padded up to 8");
  const int hp = h + (int)(pt + pb), wp = ww + (int)(pl + pr);
  const int ekh = (int)dil_h * (kh - 1) + 1, ekw = (int)dil_w * (kw - 1) + 1;
  TORCH_CHECK(hp >= ekh && wp >= ekw, "dilated filter larger than the input");
  const int oh = (hp - ekh) / (int)stride_h + 1;
  const int ow = (wp - ekw) / (int)stride_w + 1;
  auto stream = current_stream();
  // C % 8 == 0: the kernel zero-pads inline (validity check + zero-page
  // redirect in the A staging) — no materialized pad pass.  Channel
  // padding (stems) still materializes: the straddling 16-B segment
  // cannot be partially zeroed by a redirected load.
  const bool inline_pad = (c8 == c);
  torch::Tensor xp = x;
  if (!inline_pad && (pt > 0 || pb > 0 || pl > 0 || pr > 0 || c8 != c)) {
    xp = torch::empty({b, hp, wp, c8}, x.options());
    vfa_pad2d_nhwc(x.data_ptr(), xp.data_ptr(), b, h, ww, c, c8, (int)pt,
                   (int)pb, (int)pl, (int)pr, stream);
    xp = xp.permute({0, 3, 1, 2});   // logical NCHW view, CL physical
  }
  // 1 KiB zero page for out-of-image glds redirects (per device, cached)
  static std::unordered_map<int, torch::Tensor> zpages;
  static std::mutex zp_mu;
  torch::Tensor zpage;
  {
    std::lock_guard<std::mutex> lk(zp_mu);
    auto it = zpages.find((int)x.get_device());
    if (it == zpages.end()) {
      zpage = torch::zeros({512}, x.options());
      zpages.emplace((int)x.get_device(), zpage);
    } else {
      zpage = it->second;
    }
  }
  const void* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    bc = bias->contiguous().to(torch::kBFloat16);
    TORCH_CHECK(bc.numel() == kout);
    bptr = bc.data_ptr();
  }
  const void* rptr = nullptr;
  if (res.has_value()) {
    TORCH_CHECK(cl_contig(*res) && res->scalar_type() == torch::kBFloat16 &&
                res->numel() == (long long)b * oh * ow * kout,
                "residual must be CL bf16 of the output shape");
    rptr = res->data_ptr();
  }
  // optional preallocated WIDER output buffer: the epilogue writes the
  // channel slice [out_off, out_off + kout) of a (B, C_total, OH, OW) CL
  // tensor (eliminates a following cat copy)
  torch::Tensor out;
  int ldc = kout;
  void* optr;
  if (out_buf.has_value()) {
    out = *out_buf;
    TORCH_CHECK(cl_contig(out) && out.scalar_type() == torch::kBFloat16 &&
                out.size(0) == b && out.size(2) == oh && out.size(3) == ow &&
                out_off + kout <= out.size(1),
                "out buffer must be CL bf16 (B, >=off+kout, OH, OW)");
    ldc = (int)out.size(1);
    optr = static_cast<char*>(out.data_ptr()) + out_off * 2;
    // x and out may be ONE buffer (the in-place dense step) when the read
    // and written channel slices are disjoint; any other overlap of the two
    // memories is refused before anything is launched
    const char* xb = static_cast<const char*>(x.data_ptr());
    const char* ob = static_cast<const char*>(out.data_ptr());
    if (xb < ob + out.numel() * 2 && ob < xb + x.numel() * 2) {
      TORCH_CHECK(xb == ob && x.sizes() == out.sizes() &&
                  (in_off + c <= out_off || out_off + kout <= in_off),
                  "conv2d_nhwc: the read and written channel slices of one "
                  "buffer overlap");
    }
  } else {
    out = torch::empty({(long)b, oh, ow, kout}, x.options())
              .permute({0, 3, 1, 2});
    optr = out.data_ptr();
  }
  if (inline_pad)
    vfa_conv2d_nhwc(static_cast<const char*>(xp.data_ptr()) + in_off * 2,
                    w.data_ptr(), bptr, rptr,
                    zpage.data_ptr(), optr, b, h, ww, c8, oh, ow,
                    kout, kh, kw, (int)stride_h, (int)stride_w, (int)pt,
                    (int)pl, ldc, (int)act, (int)dil_h, (int)dil_w,
                    slice ? xc : c8, stream);
  else
    vfa_conv2d_nhwc(xp.data_ptr(), w.data_ptr(), bptr, rptr,
                    zpage.data_ptr(), optr, b, hp, wp, c8, oh,
                    ow, kout, kh, kw, (int)stride_h, (int)stride_w, 0, 0,
                    ldc, (int)act, (int)dil_h, (int)dil_w, c8, stream);
  return out;
}

// Output side of the transposed convs: a new channels_last (B, K, 2H, 2W)
// tensor, or the channel slice [out_off, out_off + K) of out_buf, which
// must not overlap x in memory.  Returns (tensor, first slice element, ldo).
std::tuple<torch::Tensor, void*, int> tconv_out(
    const torch::Tensor& x, c10::optional<torch::Tensor> out_buf,
    int64_t out_off, int kout) {
  const long b = x.size(0), oh = 2 * x.size(2), ow = 2 * x.size(3);
  if (!out_buf.has_value()) {
    TORCH_CHECK(out_off == 0, "out_off needs out");
    auto out = torch::empty({b, oh, ow, (long)kout}, x.options())
                   .permute({0, 3, 1, 2});
    return {out, out.data_ptr(), kout};
  }
  auto out = *out_buf;
  TORCH_CHECK(out.is_cuda() && out.dim() == 4 &&
              out.is_contiguous(torch::MemoryFormat::ChannelsLast) &&
              out.scalar_type() == torch::kBFloat16 && out.size(0) == b &&
              out.size(2) == oh && out.size(3) == ow && out_off >= 0 &&
              out_off + kout <= out.size(1),
              "out buffer must be CL bf16 (B, >=off+K_out, 2H, 2W)");
  if (x.numel() > 0 && out.numel() > 0) {
    // extent of x through its strides (it may be any strided view)
    long long span = 1;
    for (int d = 0; d < 4; ++d) span += (x.size(d) - 1) * x.stride(d);
    const char* xb = static_cast<const char*>(x.data_ptr());
    const char* ob = static_cast<const char*>(out.data_ptr());
    TORCH_CHECK(!(xb < ob + out.numel() * 2 && ob < xb + span * 2),
                "conv_transpose2d: out must not overlap x in memory");
  }
  return {out, static_cast<char*>(out.data_ptr()) + out_off * 2,
          (int)out.size(1)};
}

// P-form transposed conv (4x4, stride 2, padding 1).  x channels_last bf16;
// wp the packed (16*K_out, C) weight; in_ch > 0: x is a wider buffer and
// channels [in_off, in_off + in_ch) are read in place.
torch::Tensor conv_transpose2d_nhwc(torch::Tensor x, torch::Tensor wp,
                                    c10::optional<torch::Tensor> bias,
                                    c10::optional<torch::Tensor> out_buf,
                                    int64_t out_off, int64_t in_off,
                                    int64_t in_ch) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && cl_contig(x) &&
                  x.scalar_type() == torch::kBFloat16,
              "x must be channels_last bf16");
  const int xc = (int)x.size(1);
  const bool slice = in_ch > 0;
  if (!slice) TORCH_CHECK(in_off == 0 && in_ch == 0, "in_off needs in_ch > 0");
  const int c = slice ? (int)in_ch : xc;
  TORCH_CHECK(in_off >= 0 && in_off % 8 == 0 && c % 8 == 0 && xc % 8 == 0 &&
                  in_off + c <= xc,
              "conv_transpose2d_nhwc: in_off, in_ch and the buffer width "
              "must be multiples of 8 and the slice inside the buffer");
  TORCH_CHECK(wp.is_cuda() && wp.dim() == 2 && wp.is_contiguous() &&
                  wp.scalar_type() == torch::kBFloat16 && wp.size(1) == c &&
                  (wp.size(0) == 16 || wp.size(0) == 32),
              "packed weight must be bf16 (16*K_out, C), K_out <= 2");
  const int kout = (int)wp.size(0) / 16;
  TORCH_CHECK(vfa_tconv_lds_bytes(c, kout) <= 64 * 1024,
              "conv_transpose2d_nhwc: C too large for the LDS-resident weight");
  const int b = (int)x.size(0), h = (int)x.size(2), w = (int)x.size(3);
  const void* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    bc = bias->contiguous().to(torch::kBFloat16);
    TORCH_CHECK(bc.numel() == kout);
    bptr = bc.data_ptr();
  }
  auto [out, optr, ldo] = tconv_out(x, out_buf, out_off, kout);
  if (x.numel() == 0) return out;
  auto part = torch::empty({(long)b * h * w, 16L * kout},
                           x.options().dtype(torch::kFloat32));
  vfa_tconv_pform(static_cast<const char*>(x.data_ptr()) + in_off * 2,
                  wp.data_ptr(), bptr, part.data_ptr(), optr, b, h, w, c, xc,
                  kout, ldo, current_stream());
  return out;
}

// direct transposed conv for C <= 16: x bf16 of any strides, w (C, K_out,
// 4, 4) contiguous bf16
torch::Tensor conv_transpose2d_small(torch::Tensor x, torch::Tensor w,
                                     c10::optional<torch::Tensor> bias,
                                     c10::optional<torch::Tensor> out_buf,
                                     int64_t out_off) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 &&
                  x.scalar_type() == torch::kBFloat16 && x.size(1) <= 16,
              "x must be bf16 (B, C <= 16, H, W)");
  TORCH_CHECK(w.is_cuda() && w.dim() == 4 && w.is_contiguous() &&
                  w.scalar_type() == torch::kBFloat16 &&
                  w.size(0) == x.size(1) && w.size(1) >= 1 &&
                  w.size(1) <= 2 && w.size(2) == 4 && w.size(3) == 4,
              "weight must be contiguous bf16 (C, K_out <= 2, 4, 4)");
  const int kout = (int)w.size(1);
  const void* bptr = nullptr;
  torch::Tensor bc;
  if (bias.has_value()) {
    bc = bias->contiguous().to(torch::kBFloat16);
    TORCH_CHECK(bc.numel() == kout);
    bptr = bc.data_ptr();
  }
  auto [out, optr, ldo] = tconv_out(x, out_buf, out_off, kout);
  if (x.numel() == 0) return out;
  vfa_tconv_direct(x.data_ptr(), w.data_ptr(), bptr, optr, (int)x.size(0),
                   (int)x.size(1), (int)x.size(2), (int)x.size(3),
                   x.stride(0), x.stride(1), x.stride(2), x.stride(3), kout,
                   ldo, current_stream());
  return out;
}

// (BM, BN) of the tile conv2d_nhwc runs for M = B*OH*OW and kout — the
// same host function launch_conv calls, so tests can pin a case to a tile
std::tuple<int64_t, int64_t> conv2d_tile(int64_t m, int64_t kout) {
  TORCH_CHECK(m > 0 && kout > 0 && m <= INT_MAX && kout <= INT_MAX);
  int bm = 0, bn = 0;
  vfa_conv2d_pick_tile((int)m, (int)kout, &bm, &bn);
  return {bm, bn};
}

torch::Tensor temporal_merge(torch::Tensor y, int64_t b, int64_t kt,
                             int64_t st, int64_t p0, int64_t p1,
                             bool relu) {
  // y (B*T, kt*O, H, W) channels_last -> (B*T', O, H, W) channels_last
  TORCH_CHECK(y.is_cuda() && y.dim() == 4);
  TORCH_CHECK(cl_contig(y), "channels_last expected");
  const int bt = (int)y.size(0), cin = (int)y.size(1);
  const int h = (int)y.size(2), w = (int)y.size(3);
  const int o = cin / (int)kt, t = bt / (int)b;
  const int to = (int)((t + p0 + p1 - kt) / st + 1);
  auto out = torch::empty({(long)b * to, h, w, o}, y.options())
                 .permute({0, 3, 1, 2});
  vfa_temporal_merge(y.data_ptr(), out.data_ptr(), (int)b, t, to, (int)kt,
                     (int)st, (int)p0, o, (long long)h * w, relu ? 1 : 0,
                     dtype_tag(y), current_stream());
  return out;
}

torch::Tensor avgpool2d_nhwc(torch::Tensor x, int64_t k) {
  // x (B, C, H, W) channels_last bf16 -> (B, C, H/k, W/k) channels_last,
  // window = stride = k, floor output size (nn.AvgPool2d(k))
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && cl_contig(x),
              "x must be channels_last");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "avgpool2d_nhwc: bf16");
  TORCH_CHECK(x.size(1) % 8 == 0, "avgpool2d_nhwc: C % 8 == 0 required");
  TORCH_CHECK(k >= 1 && k <= x.size(2) && k <= x.size(3),
              "avgpool2d_nhwc: window larger than the input");
  const int64_t oh = x.size(2) / k, ow = x.size(3) / k;
  auto out = torch::empty({x.size(0), oh, ow, x.size(1)}, x.options())
                 .permute({0, 3, 1, 2});
  vfa_avgpool2d_nhwc(x.data_ptr(), out.data_ptr(), x.size(0), (int)x.size(1),
                     (int)x.size(2), (int)x.size(3), (int)oh, (int)ow, (int)k,
                     current_stream());
  return out;
}

torch::Tensor attnpool_tokens(torch::Tensor x, torch::Tensor pos) {
  // x (B, HW, C) bf16, pos (HW+1, C) bf16 -> t (B, HW+1, C) bf16
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.is_contiguous());
  TORCH_CHECK(pos.is_cuda() && pos.dim() == 2 && pos.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              pos.scalar_type() == torch::kBFloat16, "attnpool_tokens: bf16");
  const int64_t hw = x.size(1), c = x.size(2);
  TORCH_CHECK(hw >= 1 && c % 8 == 0, "attnpool_tokens: C % 8 == 0 required");
  TORCH_CHECK(pos.size(0) == hw + 1 && pos.size(1) == c,
              "positional embedding must be (HW+1, C)");
  auto t = torch::empty({x.size(0), hw + 1, c}, x.options());
  vfa_attnpool_tokens(x.data_ptr(), pos.data_ptr(), t.data_ptr(), x.size(0),
                      (int)hw, (int)c, current_stream());
  return t;
}

torch::Tensor attention_pool(torch::Tensor q, torch::Tensor kv,
                             int64_t heads) {
  // q (B, C) bf16, kv (B, L, 2C) bf16 packed [k | v], C == heads * 64
  TORCH_CHECK(q.is_cuda() && q.dim() == 2 && q.is_contiguous());
  TORCH_CHECK(kv.is_cuda() && kv.dim() == 3 && kv.is_contiguous());
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 &&
              kv.scalar_type() == torch::kBFloat16, "attention_pool: bf16");
  const int64_t b = q.size(0), c = q.size(1), l = kv.size(1);
  TORCH_CHECK(heads >= 1 && c == heads * 64,
              "attention_pool covers head_dim 64");
  TORCH_CHECK(kv.size(0) == b && kv.size(2) == 2 * c && l >= 1,
              "kv must be (B, L>=1, 2C)");
  auto out = torch::empty({b, c}, q.options());
  vfa_attention_pool_d64(q.data_ptr(), kv.data_ptr(), out.data_ptr(), b,
                         (int)heads, (int)l, 0.125f, current_stream());
  return out;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("quick_gelu", &quick_gelu);
  m.def("gelu_tanh", &gelu_tanh);
  m.def("layer_norm", &layer_norm);
  m.def("bilinear_warp", &bilinear_warp);
  m.def("grid_sample_bilinear", &grid_sample_bilinear);
  m.def("pwc_correlation", &pwc_correlation);
  m.def("mhsa", &mhsa);
  m.def("flash_qkv", &flash_qkv);
  m.def("mfma_gemm16", &mfma_gemm16);
  m.def("layer_norm_residual", &layer_norm_residual);
  m.def("clip_embed_ln", &clip_embed_ln);
  m.def("u8_chw_norm", &u8_chw_norm);
  m.def("corr_lookup", &corr_lookup);
  m.def("convex_upsample", &convex_upsample);
  m.def("gru_zr", &gru_zr);
  m.def("gru_out", &gru_out);
  m.def("instance_norm2d", &instance_norm2d);
  m.def("maxpool3d_same", &maxpool3d_same);
  m.def("maxpool2d_same", &maxpool2d_same);
  m.def("linear_act", &linear_act);
  m.def("linear_res_stats", &linear_res_stats);
  m.def("linear_ln_act", &linear_ln_act);
  m.def("conv2d_nhwc", &conv2d_nhwc);
  m.def("conv2d_tile", &conv2d_tile);
  m.def("conv_transpose2d_nhwc", &conv_transpose2d_nhwc);
  m.def("conv_transpose2d_small", &conv_transpose2d_small);
  m.def("bilinear_warp_nhwc", &bilinear_warp_nhwc);
  m.def("pwc_correlation_nhwc", &pwc_correlation_nhwc);
  m.def("temporal_merge", &temporal_merge);
  m.def("avgpool2d_nhwc", &avgpool2d_nhwc);
  m.def("attnpool_tokens", &attnpool_tokens);
  m.def("attention_pool", &attention_pool);
  m.attr("gfx_arch") = "gfx950";
}
