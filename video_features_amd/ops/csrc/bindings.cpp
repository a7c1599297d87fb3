// Python bindings for the VFA gfx950 HIP kernels (torch extension ABI).
// Kernels live in the sibling .hip TUs behind a C ABI (vfa_api.h, the one
// declaration both sides compile against) so this slow, torch-header-heavy
// TU stays apart from the device code.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <mutex>
#include <unordered_map>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "vfa_api.h"

namespace {

int dtype_tag(torch::ScalarType s) {
  switch (s) {
    case torch::kFloat32: return 0;
    case torch::kBFloat16: return 1;
    case torch::kFloat16: return 2;
    default:
      TORCH_CHECK(false, "unsupported dtype ", s);
  }
}

int dtype_tag(const torch::Tensor& t) { return dtype_tag(t.scalar_type()); }

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// channels_last strides (a tensor with C == 1 or H == W == 1 is both)
bool cl_contig(const torch::Tensor& t) {
  return t.is_contiguous(torch::MemoryFormat::ChannelsLast);
}

// 4-D, channels_last and NOT also plain contiguous
bool cl_only(const torch::Tensor& t) {
  return t.dim() == 4 && cl_contig(t) && !t.is_contiguous();
}

// the layout an op's nhwc flag promises for t
void check_layout(const torch::Tensor& t, bool nhwc) {
  TORCH_CHECK(nhwc ? cl_contig(t) : t.is_contiguous(),
              nhwc ? "channels_last expected" : "contiguous expected");
}

// (b, c, h, w) view of newly allocated NHWC memory
torch::Tensor empty_nhwc(int64_t b, int64_t c, int64_t h, int64_t w,
                         const torch::TensorOptions& opts) {
  return torch::empty({b, h, w, c}, opts).permute({0, 3, 1, 2});
}

// optional bias of n elements as contiguous bf16: (keep-alive, pointer or
// nullptr)
std::pair<torch::Tensor, const void*> bf16_bias(
    const c10::optional<torch::Tensor>& bias, int64_t n) {
  if (!bias.has_value()) return {torch::Tensor(), nullptr};
  auto bc = bias->contiguous().to(torch::kBFloat16);
  TORCH_CHECK(bc.numel() == n, "bias must have ", n, " elements");
  return {bc, bc.data_ptr()};
}

// Where a kernel writes its k NHWC bf16 output channels: the channel slice
// [out_off, out_off + k) of out_buf, a channels_last bf16 (b, >= out_off + k,
// oh, ow) buffer, or a new channels_last (b, k, oh, ow) tensor.  Returns
// (tensor, first slice element, pixel stride in elements).  Any rule about
// out_buf overlapping an input is the caller's.
std::tuple<torch::Tensor, void*, int> out_slice(
    const c10::optional<torch::Tensor>& out_buf, int64_t out_off, int64_t b,
    int64_t k, int64_t oh, int64_t ow, const torch::TensorOptions& opts) {
  if (!out_buf.has_value()) {
    auto out = empty_nhwc(b, k, oh, ow, opts);
    return {out, out.data_ptr(), (int)k};
  }
  auto out = *out_buf;
  TORCH_CHECK(out.is_cuda() && out.dim() == 4 && cl_contig(out) &&
              out.scalar_type() == torch::kBFloat16 && out.size(0) == b &&
              out.size(2) == oh && out.size(3) == ow && out_off >= 0 &&
              out_off + k <= out.size(1),
              "out buffer must be channels_last bf16 (B, >= out_off + ", k,
              ", ", oh, ", ", ow, ")");
  return {out, static_cast<char*>(out.data_ptr()) + out_off * 2,
          (int)out.size(1)};
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
  if (x.numel() == 0) return out;
  vfa_layer_norm(x.data_ptr(), wc.data_ptr(), bc.data_ptr(), out.data_ptr(),
                 x.numel() / d, d, (float)eps, dtype_tag(x), current_stream());
  return out;
}

// (T, P, W) patch embeddings + cls (W) + pos (P+1, W) -> ln_pre'd tokens
// (T, P+1, W); see EmbedSrc in layernorm.hip
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
  if (out.numel() == 0) return out;
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
  auto [out, optr, ldo] = out_slice(out_buf, out_off, b, 81, h, w,
                                    f1.options());
  vfa_pwc_correlation_nhwc(f1.data_ptr(), f2.data_ptr(), optr, b, c, h, w,
                           ldo, leaky ? 1 : 0, current_stream());
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
    auto [out, optr, ldo] = out_slice(out_buf, out_off, b, 81, h, w, opts);
    vfa_pwc_correlation(f1.data_ptr(), f1p.data_ptr(), f2p.data_ptr(), optr,
                        b, c, h, w, tag, ldo, leaky ? 1 : 0, stream);
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
  TORCH_CHECK(w.numel() == d && b.numel() == d, "affine shape mismatch");
  auto wc = w.contiguous().to(x.scalar_type());
  auto bc = b.contiguous().to(x.scalar_type());
  auto y = torch::empty_like(x);
  auto s = torch::empty_like(x);
  if (x.numel() == 0) return {y, s};
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

// (T, C, H, W) -> (T, (H/p)*(W/p), C*p*p); see patchify_kernel
torch::Tensor patchify(torch::Tensor x, int64_t p) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4,
              "patchify: contiguous (T, C, H, W) expected");
  const int64_t es = x.element_size();
  const int64_t t = x.size(0), c = x.size(1), h = x.size(2), w = x.size(3);
  TORCH_CHECK((es == 2 || es == 4) && p > 0 && (p * es) % 16 == 0 &&
              h % p == 0 && w % p == 0,
              "patchify: itemsize 2 or 4, p * itemsize % 16 == 0 and "
              "H, W multiples of p required");
  TORCH_CHECK(c * h * w * es / 16 < (1LL << 31), "patchify: frame too large");
  auto out = torch::empty({t, (h / p) * (w / p), c * p * p}, x.options());
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
              (uintptr_t)out.data_ptr() % 16 == 0,
              "patchify: 16-B aligned tensors required");
  vfa_patchify(x.data_ptr(), out.data_ptr(), t, (int)c, (int)h, (int)w,
               (int)p, (int)es, current_stream());
  return out;
}

torch::Tensor flash_qkv(torch::Tensor qkv, double scale, int64_t variant) {
  // qkv: (B, N, 3, H, D) bf16 contiguous, D == 64 -> out (B, N, H*D)
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 5);
  TORCH_CHECK(qkv.size(2) == 3 && qkv.size(4) == 64,
              "flash_qkv covers head_dim 64");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16);
  const int b = (int)qkv.size(0), n = (int)qkv.size(1);
  const int h = (int)qkv.size(3);
  auto out = torch::empty({b, n, h * 64L}, qkv.options());
  TORCH_CHECK(variant == 0 || variant == 1, "flash_qkv: variant 0 or 1");
  TORCH_CHECK((int64_t)b * h * 2 < (1LL << 31), "flash_qkv: too many pairs");
  vfa_flash_qkv(qkv.data_ptr(), out.data_ptr(), b, n, h, (float)scale,
                (int)variant, current_stream());
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
  const int tag = dtype_tag(out_dtype);   // raises before anything launches
  TORCH_CHECK(coords.is_cuda() && coords.dim() == 4 && coords.size(1) == 2);
  auto cc = coords.to(torch::kFloat32).contiguous();
  const long long b = coords.size(0);
  const int h = (int)coords.size(2), w = (int)coords.size(3);
  const long long npix = b * h * w;
  CorrPyramid pyr;
  long long lds_floats = 0;
  for (int l = 0; l < levels; ++l) {
    auto& t = pyramid[l];
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                t.scalar_type() == torch::kFloat32);
    TORCH_CHECK(t.size(0) == npix && t.size(1) == 1, "plane-per-pixel");
    pyr.hs[l] = (int)t.size(2);
    pyr.ws[l] = (int)t.size(3);
    pyr.lvl[l] = t.data_ptr();
    lds_floats += pyr.hs[l] * pyr.ws[l];
  }
  for (int l = levels; l < 4; ++l) {
    pyr.hs[l] = pyr.ws[l] = 1;
    pyr.lvl[l] = pyr.lvl[levels - 1];
  }
  const int ctot = levels * 81;
  auto opts = coords.options().dtype(out_dtype);
  auto out = nhwc ? empty_nhwc(b, ctot, h, w, opts)
                  : torch::empty({b, ctot, h, w}, opts);
  vfa_corr_lookup(pyr, cc.data_ptr(), out.data_ptr(), levels, npix, h * w,
                  (int)((lds_floats <= 16384 && !force_gmem) ? lds_floats : 0),
                  nhwc ? 1 : 0, tag, current_stream());
  return out;
}

torch::Tensor corr_lookup_otf(torch::Tensor f1,
                              std::vector<torch::Tensor> f2_levels,
                              torch::Tensor coords, bool nhwc,
                              torch::ScalarType out_dtype) {
  // f1 (B, H, W, D) and f2_levels[l] (B, h_l, w_l, D): fp32, pixel-major;
  // coords (B, 2, H, W) fp32 pixel units at level 0.  Returns what
  // corr_lookup returns for the all-pairs pyramid of the same features.
  const int levels = (int)f2_levels.size();
  TORCH_CHECK(levels >= 1 && levels <= 4, "1..4 feature levels");
  const int tag = dtype_tag(out_dtype);   // raises before anything launches
  TORCH_CHECK(f1.is_cuda() && f1.dim() == 4 && f1.is_contiguous() &&
              f1.scalar_type() == torch::kFloat32,
              "f1 must be a contiguous f32 (B, H, W, D) GPU tensor");
  const long long b = f1.size(0);
  const int h = (int)f1.size(1), w = (int)f1.size(2);
  const int d = (int)f1.size(3);
  TORCH_CHECK(d % 32 == 0 && d >= 32 && d <= 256,
              "D must be a multiple of 32, at most 256");
  TORCH_CHECK(coords.is_cuda() && coords.dim() == 4 &&
              coords.is_contiguous() &&
              coords.scalar_type() == torch::kFloat32 &&
              coords.size(0) == b && coords.size(1) == 2 &&
              coords.size(2) == h && coords.size(3) == w,
              "coords must be a contiguous f32 (B, 2, H, W) GPU tensor");
  TORCH_CHECK((long long)h * w < (1LL << 31), "frame too large");
  CorrPyramid lv;
  for (int l = 0; l < levels; ++l) {
    auto& t = f2_levels[l];
    TORCH_CHECK(t.is_cuda() && t.dim() == 4 && t.is_contiguous() &&
                t.scalar_type() == torch::kFloat32 &&
                t.get_device() == f1.get_device(),
                "f2 levels must be contiguous f32 GPU tensors");
    TORCH_CHECK(t.size(0) == b && t.size(3) == d && t.size(1) >= 1 &&
                t.size(2) >= 1 && t.size(1) <= h && t.size(2) <= w,
                "f2 level ", l, " must be (B, 1..H, 1..W, D)");
    lv.hs[l] = (int)t.size(1);
    lv.ws[l] = (int)t.size(2);
    lv.lvl[l] = t.data_ptr();
  }
  for (int l = levels; l < 4; ++l) {
    lv.hs[l] = lv.ws[l] = 1;
    lv.lvl[l] = lv.lvl[levels - 1];
  }
  const int ctot = levels * 81;
  auto opts = coords.options().dtype(out_dtype);
  auto out = nhwc ? empty_nhwc(b, ctot, h, w, opts)
                  : torch::empty({b, ctot, h, w}, opts);
  vfa_corr_otf(f1.data_ptr(), lv, coords.data_ptr(), out.data_ptr(), levels,
               b * h * w, h * w, d, nhwc ? 1 : 0, tag, current_stream());
  return out;
}

torch::Tensor convex_upsample(torch::Tensor flow, torch::Tensor mask,
                              bool nhwc) {
  TORCH_CHECK(flow.is_cuda() && flow.dim() == 4 && flow.size(1) == 2);
  TORCH_CHECK(mask.dim() == 4 && mask.size(1) == 576);
  TORCH_CHECK(mask.scalar_type() == flow.scalar_type());
  check_layout(flow, nhwc);
  check_layout(mask, nhwc);
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
  for (const auto* t : {&zr, &hx, &rhx}) check_layout(*t, nhwc);
  auto z = nhwc ? empty_nhwc(b, c, zr.size(2), zr.size(3), zr.options())
                : torch::empty({b, c, zr.size(2), zr.size(3)}, zr.options());
  vfa_gru_zr(zr.data_ptr(), hx.data_ptr(), rhx.data_ptr(), z.data_ptr(), b,
             c, ctot - c, hw, nhwc ? 1 : 0, dtype_tag(zr), current_stream());
  return z;
}

void gru_out(torch::Tensor q, torch::Tensor z, torch::Tensor hx, bool nhwc) {
  const int b = (int)q.size(0), c = (int)q.size(1), ctot = (int)hx.size(1);
  const long long hw = (long long)q.size(2) * q.size(3);
  check_layout(q, nhwc);
  check_layout(hx, nhwc);
  vfa_gru_out(q.data_ptr(), z.data_ptr(), hx.data_ptr(), b, c, ctot - c, hw,
              nhwc ? 1 : 0, dtype_tag(q), current_stream());
}

torch::Tensor instance_norm2d(torch::Tensor x, double eps, bool relu,
                              bool nhwc) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4);
  if (x.numel() == 0) return torch::empty_like(x);  // no layout to speak of
  check_layout(x, nhwc);
  auto out = torch::empty_like(x);
  vfa_instance_norm2d(x.data_ptr(), out.data_ptr(), (int)x.size(0),
                      (int)x.size(1), (int)(x.size(2) * x.size(3)),
                      (float)eps, relu ? 1 : 0, nhwc ? 1 : 0, dtype_tag(x),
                      current_stream());
  return out;
}

// nd = 2 or 3 pooled dims: the last nd of x
PoolGeom pool_geom(const torch::Tensor& x, int nd,
                   const std::vector<int64_t>& kernel,
                   const std::vector<int64_t>& stride,
                   const std::vector<int64_t>& pad_front,
                   const std::vector<int64_t>& out_sz) {
  for (const auto* v : {&kernel, &stride, &pad_front, &out_sz})
    TORCH_CHECK((int)v->size() >= nd, "pool: ", nd, " values per argument");
  PoolGeom g{};
  for (int i = 0; i < nd; ++i) {
    g.in[i] = (int)x.size(x.dim() - nd + i);
    g.out[i] = (int)out_sz[i];
    g.k[i] = (int)kernel[i];
    g.s[i] = (int)stride[i];
    g.pad[i] = (int)pad_front[i];
  }
  return g;
}

torch::Tensor maxpool3d_same(torch::Tensor x, std::vector<int64_t> kernel,
                             std::vector<int64_t> stride,
                             std::vector<int64_t> pad_front,
                             std::vector<int64_t> out_sz) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 5);
  const long long bc = x.size(0) * x.size(1);
  auto out = torch::empty({x.size(0), x.size(1), out_sz[0], out_sz[1],
                           out_sz[2]}, x.options());
  vfa_maxpool3d_same(x.data_ptr(), out.data_ptr(), bc,
                     pool_geom(x, 3, kernel, stride, pad_front, out_sz),
                     dtype_tag(x), current_stream());
  return out;
}

torch::Tensor maxpool2d_same(torch::Tensor x, std::vector<int64_t> kernel,
                             std::vector<int64_t> stride,
                             std::vector<int64_t> pad_front,
                             std::vector<int64_t> out_sz, bool nhwc) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4);
  check_layout(x, nhwc);
  auto out = nhwc
      ? empty_nhwc(x.size(0), x.size(1), out_sz[0], out_sz[1], x.options())
      : torch::empty({x.size(0), x.size(1), out_sz[0], out_sz[1]},
                     x.options());
  vfa_maxpool2d_same(x.data_ptr(), out.data_ptr(), x.size(0), (int)x.size(1),
                     pool_geom(x, 2, kernel, stride, pad_front, out_sz),
                     nhwc ? 1 : 0, dtype_tag(x), current_stream());
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
  auto [bc, bptr] = bf16_bias(bias, n);
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

// name of the kernel route linear_act takes for (m, n, k, act) — the same
// host function the launchers call, so tests can pin a case to a kernel.
// The thin route reads "thin:<nch>" with its N-chunk.
std::string linear_route(int64_t m, int64_t n, int64_t k, int64_t act) {
  TORCH_CHECK(m > 0 && n > 0 && k > 0 && m <= INT_MAX && n <= INT_MAX &&
              k <= INT_MAX && k % 8 == 0 && act >= 0 && act <= 4);
  static const char* const names[] = {"thin", "8p", "256p", "256p+edge",
                                      "big_guard", "small"};
  int nch = 0;
  const int r = vfa_linear_route((int)m, (int)n, (int)k, (int)act, &nch);
  std::string s = names[r];
  return r == VFA_ROUTE_THIN ? s + ":" + std::to_string(nch) : s;
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
  auto [bc, bptr] = bf16_bias(bias, n);
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
    xp = empty_nhwc(b, c8, hp, wp, x.options());
    vfa_pad2d_nhwc(x.data_ptr(), xp.data_ptr(), b, h, ww, c, c8, (int)pt,
                   (int)pb, (int)pl, (int)pr, stream);
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
  auto [bc, bptr] = bf16_bias(bias, kout);
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
  auto [out, optr, ldc] = out_slice(out_buf, out_off, b, kout, oh, ow,
                                    x.options());
  if (out_buf.has_value()) {
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
  }
  ConvGeom g;
  g.b = b;
  g.hp = inline_pad ? h : hp;    // a materialized pad leaves none inline
  g.wp = inline_pad ? ww : wp;
  g.cin = c8;
  g.oh = oh;
  g.ow = ow;
  g.kout = kout;
  g.kh = kh;
  g.kw = kw;
  g.sh = (int)stride_h;
  g.sw = (int)stride_w;
  g.pt = inline_pad ? (int)pt : 0;
  g.pl = inline_pad ? (int)pl : 0;
  g.kr = kh * kw * c8;
  ConvAddr a;
  a.dh = (int)dil_h;
  a.dw = (int)dil_w;
  a.ldx = slice ? xc : c8;       // a slice is always inline_pad (c % 8 == 0)
  vfa_conv2d_nhwc(static_cast<const char*>(xp.data_ptr()) + in_off * 2,
                  w.data_ptr(), bptr, rptr, zpage.data_ptr(), optr, g, a, ldc,
                  (int)act, stream);
  return out;
}

// Output side of the transposed convs: out_slice for a (B, K, 2H, 2W)
// result, where out_buf must not overlap x in memory.
std::tuple<torch::Tensor, void*, int> tconv_out(
    const torch::Tensor& x, const c10::optional<torch::Tensor>& out_buf,
    int64_t out_off, int kout) {
  if (!out_buf.has_value()) TORCH_CHECK(out_off == 0, "out_off needs out");
  auto res = out_slice(out_buf, out_off, x.size(0), kout, 2 * x.size(2),
                       2 * x.size(3), x.options());
  const auto& out = std::get<0>(res);
  if (out_buf.has_value() && x.numel() > 0 && out.numel() > 0) {
    // extent of x through its strides (it may be any strided view)
    long long span = 1;
    for (int d = 0; d < 4; ++d) span += (x.size(d) - 1) * x.stride(d);
    const char* xb = static_cast<const char*>(x.data_ptr());
    const char* ob = static_cast<const char*>(out.data_ptr());
    TORCH_CHECK(!(xb < ob + out.numel() * 2 && ob < xb + span * 2),
                "conv_transpose2d: out must not overlap x in memory");
  }
  return res;
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
  auto [bc, bptr] = bf16_bias(bias, kout);
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
  auto [bc, bptr] = bf16_bias(bias, kout);
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
  auto out = empty_nhwc(b * to, o, h, w, y.options());
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
  auto out = empty_nhwc(x.size(0), x.size(1), oh, ow, x.options());
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
  m.def("flash_qkv", &flash_qkv, py::arg("qkv"), py::arg("scale"),
        py::arg("variant") = 0);
  m.def("mfma_gemm16", &mfma_gemm16);
  m.def("layer_norm_residual", &layer_norm_residual);
  m.def("clip_embed_ln", &clip_embed_ln);
  m.def("u8_chw_norm", &u8_chw_norm);
  m.def("patchify", &patchify);
  m.def("corr_lookup", &corr_lookup);
  m.def("corr_lookup_otf", &corr_lookup_otf);
  m.def("convex_upsample", &convex_upsample);
  m.def("gru_zr", &gru_zr);
  m.def("gru_out", &gru_out);
  m.def("instance_norm2d", &instance_norm2d);
  m.def("maxpool3d_same", &maxpool3d_same);
  m.def("maxpool2d_same", &maxpool2d_same);
  m.def("linear_act", &linear_act);
  m.def("linear_route", &linear_route);
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
