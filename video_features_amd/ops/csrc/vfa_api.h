// The C-linkage launcher ABI between bindings.cpp and the .hip TUs: the ONE
// declaration of every vfa_* function.  vfa_common.h includes it, so each
// definition is checked against its declaration when its .hip compiles (a
// mismatch is "conflicting types"), and bindings.cpp calls through the same
// text.  A new launcher is declared here, defined in its .hip, and gets no
// local prototype anywhere.
//
// dtype: 0 f32, 1 bf16, 2 f16 (VfaDType).  nhwc / relu / leaky: 0 or 1.
// act: 0 none, 1 relu, 2 quick_gelu, 3 gelu_tanh, 4 leaky_relu(0.1).
#pragma once
#include <hip/hip_runtime.h>

// ----------------------------------------------------------------- structs
// conv2d_nhwc geometry; passed to the kernel by value (layout is ABI)
struct ConvGeom {
  int b, hp, wp, cin;       // input dims as addressed (REAL h/w when the
                            // kernel pads inline; pre-padded dims when the
                            // pad was materialized, with pt = pl = 0)
  int oh, ow, kout;         // output
  int kh, kw, sh, sw;       // filter / stride
  int pt, pl;               // inline zero-pad (top/left); bottom/right are
                            // implied by oh/ow + the validity check
  int kr;                   // KH*KW*C
};

// tap / pixel addressing beyond the plain conv
struct ConvAddr {
  int dh, dw;               // dilation
  int ldx;                  // input pixel stride in elements (>= cin; cin
                            // stays the width the K index runs over)
};

// RAFT correlation pyramid: level l is (npix, 1, hs[l], ws[l]) f32; unused
// levels repeat the last pointer with hs = ws = 1.  vfa_corr_otf passes the
// pooled feature levels (B, hs[l], ws[l], d) in the same struct.
struct CorrPyramid {
  const void* lvl[4];
  int hs[4], ws[4];
};

// SAME-padded max pool; index 0..2 = (t, h, w) for 3-D, 0..1 = (h, w) for 2-D
struct PoolGeom {
  int in[3], out[3];        // input / output size
  int k[3], s[3];           // window / stride
  int pad[3];               // padding in front (the rest falls behind)
};

extern "C" {

// ------------------------------------------------------- elementwise.hip
// out = act(in), n elements
void vfa_quick_gelu(const void* in, void* out, long long n, int dtype,
                    hipStream_t stream);
void vfa_gelu_tanh(const void* in, void* out, long long n, int dtype,
                   hipStream_t stream);

// --------------------------------------------------------- layernorm.hip
// rows x d, affine w / b of d elements in the same dtype
void vfa_layer_norm(const void* in, const void* w, const void* b, void* out,
                    long long rows, int d, float eps, int dtype,
                    hipStream_t stream);
// s_out = x + res, y = LayerNorm(s_out)
void vfa_layer_norm_residual(const void* x, const void* res, const void* w,
                             const void* b, void* y, void* s_out,
                             long long rows, int d, float eps, int dtype,
                             hipStream_t stream);
// rows = frames * (p + 1); d % 8 == 0 (checked by the binding)
void vfa_clip_embed_ln(const void* pe, const void* cls, const void* pos,
                       const void* w, const void* b, void* out,
                       long long rows, int p, int d, float eps, int dtype,
                       hipStream_t stream);

// -------------------------------------------------------------- warp.hip
// x, out (b, c, h, w) contiguous; flow (b, 2, h, w) in x's dtype
void vfa_bilinear_warp(const void* x, const void* flow, void* out, int b,
                       int c, int h, int w, int dtype, hipStream_t stream);
// x, out: channels_last bf16 (b, c, h, w) with c % 8 == 0; flow: bf16,
// element strides (fb, fc, fh, fw)
void vfa_bilinear_warp_nhwc(const void* x, const void* flow, void* out, int b,
                            int c, int h, int w, long long fb, long long fc,
                            long long fh, long long fw, float scale,
                            hipStream_t stream);
// x (n, c, h, w), coords (n, ho, wo, 2) in pixels -> out (n, c, ho, wo)
void vfa_grid_sample(const void* x, const void* coords, void* out,
                     long long n, int c, int h, int w, int ho, int wo,
                     int dtype, hipStream_t stream);

// ------------------------------------------------------- correlation.hip
// (b, c, h, w) NCHW -> (b, h + 8, w + 8, c) zero-padded NHWC
void vfa_corr_repack(const void* in, void* out, int b, int c, int h, int w,
                     int dtype, hipStream_t stream);
// f1: NCHW original; f1p/f2p: padded NHWC (from vfa_corr_repack);
// out: (B, 81, H, W) float32 when ldo == 0; with ldo > 0 the first of the
// 81 bf16 slice channels of pixel 0 in an NHWC buffer of pixel stride ldo
void vfa_pwc_correlation(const void* f1, const void* f1p, const void* f2p,
                         void* out, int b, int c, int h, int w, int dtype,
                         int ldo, int leaky, hipStream_t stream);
// f1, f2: unpadded channels_last bf16 (B, C, H, W), C <= 256; out: the first
// of the 81 bf16 slice channels of pixel 0 in an NHWC buffer of pixel
// stride ldo > 0.  No repack and no padded copy.
void vfa_pwc_correlation_nhwc(const void* f1, const void* f2, void* out,
                              int b, int c, int h, int w, int ldo, int leaky,
                              hipStream_t stream);

// ------------------------------------------------------------- tconv.hip
// bytes of dynamic LDS tconv_p_kernel needs for c input channels
long long vfa_tconv_lds_bytes(int c, int kout);
// x: first element of the input slice (pixel stride ldx, c % 8 == 0);
// wp: (16*kout, c) packed bf16; part: (b*h*w, 16*kout) f32 workspace;
// out: first element of the output slice (pixel stride ldo)
void vfa_tconv_pform(const void* x, const void* wp, const void* bias,
                     void* part, void* out, int b, int h, int w, int c,
                     int ldx, int kout, int ldo, hipStream_t stream);
// x: bf16 (b, c <= 16, h, w) with element strides (sb, sc, sh, sw); wgt
// (c, kout, 4, 4) contiguous bf16; out as for vfa_tconv_pform
void vfa_tconv_direct(const void* x, const void* wgt, const void* bias,
                      void* out, int b, int c, int h, int w, long long sb,
                      long long sc, long long sh, long long sw, int kout,
                      int ldo, hipStream_t stream);

// --------------------------------------------------------- attention.hip
// q, k, v, out (bh, n <= 64, d <= 128)
void vfa_mhsa_small(const void* q, const void* k, const void* v, void* out,
                    int bh, int n, int d, float scale, int dtype,
                    hipStream_t stream);

// --------------------------------------------------- attention_flash.hip
// qkv (b, n, 3, h, 64) bf16 -> out (b, n, h*64).  variant 0: the kernel the
// shape is routed to (n <= 64: flash_qkv_regs_kernel); 1: the general
// flash_qkv_kernel at any n
void vfa_flash_qkv(const void* qkv, void* out, int b, int n, int h,
                   float scale, int variant, hipStream_t stream);
// d (16, 16) = a (16, 32) @ b (32, 16), f32 in and out: the MFMA self-test
void vfa_mfma_gemm16(const void* a, const void* b, void* d,
                     hipStream_t stream);

// -------------------------------------------------------- preprocess.hip
// in (t, h, w, 3) u8 -> out (t, 3, h, w) = (in / 255 - mean) / std;
// mean / std: 3 host floats; dtype f32 or bf16
void vfa_u8_chw_norm(const void* in, void* out, long long t, int h, int w,
                     const float* mean, const float* std, int dtype,
                     hipStream_t stream);
// in (t, c, h, w) -> out (t, (h/p)*(w/p), c*p*p), K order (c, py, px);
// itemsize 2 or 4, p*itemsize % 16 == 0, h % p == w % p == 0, 16-B aligned
// pointers, c*h*w*itemsize/16 < 2^31
void vfa_patchify(const void* in, void* out, long long t, int c, int h, int w,
                  int p, int itemsize, hipStream_t stream);

// -------------------------------------------------------------- raft.hip
// coords (B, 2, H, W) f32 pixel units at level 0, hw = H*W, npix = B*hw;
// out (B, levels*81, H, W) in dtype; lds_floats: sum of the level planes'
// sizes when they fit LDS, 0 for the global-memory kernel
void vfa_corr_lookup(const CorrPyramid& pyr, const void* coords, void* out,
                     int levels, long long npix, int hw, int lds_floats,
                     int nhwc, int dtype, hipStream_t stream);
// The same lookup computed from the features (no all-pairs volume): f1
// (B, H, W, d) f32 and f2.lvl[l] (B, hs[l], ws[l], d) f32, the avg-pooled
// second feature map, both pixel-major; d % 32 == 0, d <= 256, every level
// at least 1x1; coords / out / hw / npix as above
void vfa_corr_otf(const void* f1, const CorrPyramid& f2, const void* coords,
                  void* out, int levels, long long npix, int hw, int d,
                  int nhwc, int dtype, hipStream_t stream);
// flow (b, 2, h, w), mask (b, 576, h, w) -> out (b, 2, 8h, 8w) contiguous
void vfa_convex_upsample(const void* flow, const void* mask, void* out, int b,
                         int h, int w, int nhwc, int dtype,
                         hipStream_t stream);
// zr (b, 2c, hw) conv output; hx / rhx (b, c + cx, hw): writes
// sigmoid(r) * h into rhx[:, :c] and z = sigmoid(z) (b, c, hw)
void vfa_gru_zr(const void* zr, const void* hx, void* rhx, void* z, int b,
                int c, int cx, long long hw, int nhwc, int dtype,
                hipStream_t stream);
// hx[:, :c] = (1 - z) * hx[:, :c] + z * tanh(q)
void vfa_gru_out(const void* q, const void* z, void* hx, int b, int c, int cx,
                 long long hw, int nhwc, int dtype, hipStream_t stream);

// ------------------------------------------------------ instancenorm.hip
// x, out (b, c, hw), no affine; relu fused when set
void vfa_instance_norm2d(const void* x, void* out, int b, int c, int hw,
                         float eps, int relu, int nhwc, int dtype,
                         hipStream_t stream);

// ------------------------------------------------------------ pool3d.hip
// x (bc, in[0..2]) -> out (bc, out[0..2])
void vfa_maxpool3d_same(const void* x, void* out, long long bc,
                        const PoolGeom& g, int dtype, hipStream_t stream);
// x (n, c, in[0..1]) -> out (n, c, out[0..1])
void vfa_maxpool2d_same(const void* x, void* out, long long n, int c,
                        const PoolGeom& g, int nhwc, int dtype,
                        hipStream_t stream);
// x (n, c, ih, iw) channels_last bf16, c % 8 == 0; window = stride = k
void vfa_avgpool2d_nhwc(const void* x, void* out, long long n, int c, int ih,
                        int iw, int oh, int ow, int k, hipStream_t stream);

// -------------------------------------------------------------- gemm.hip
// c (m, n) = act(a (m, k) @ w (n, k)^T + bias [+ res]), all bf16
void vfa_linear_act(const void* a, const void* w, const void* bias,
                    const void* res, void* c, int m, int n, int k, int act,
                    hipStream_t stream);
// The kernel vfa_linear_act runs for an (m, n, k) problem with activation
// id act — the function its launchers call (also bound to Python as
// linear_route, so a test can pin a shape).  *nch: the thin kernel's
// N-chunk, 0 on every other route.
enum {
  VFA_ROUTE_THIN = 0,       // linear_thin_kernel
  VFA_ROUTE_8P = 1,         // linear8p_kernel
  VFA_ROUTE_256P = 2,       // linear256p_kernel, every tile
  VFA_ROUTE_256P_EDGE = 3,  // linear256p_kernel + guarded last tile column
  VFA_ROUTE_BIG_GUARD = 4,  // 256^2 linear_act_kernel (ragged K or n % 8)
  VFA_ROUTE_SMALL = 5,      // 128^2 linear_act_kernel
};
int vfa_linear_route(int m, int n, int k, int act, int* nch);
// s = a @ w^T + bias + res (bf16) and, per row of s and 256-column group
// (tile column), the (mean, M2) of the rounded values: part (M, N/256)
// float2.  Full tiles only (m % 256 == n % 256 == k % 64 == 0; the binding
// checks).
void vfa_linear_res_stats(const void* a, const void* w, const void* bias,
                          const void* res, void* c, void* part, int m, int n,
                          int k, hipStream_t stream);
// c = act(rstd * (a @ w^T - mean * ln_c) + ln_b): LayerNorm folded into the
// linear layer (w, ln_c, ln_b from ops.fold_ln_linear), a un-normalised,
// stats (M, groups) float2 partials of a's rows over k / groups columns
// each.  Full tiles only, as above.
void vfa_linear_ln_act(const void* a, const void* stats, int groups,
                       const void* w, const void* ln_c, const void* ln_b,
                       void* c, int m, int n, int k, float eps, int act,
                       hipStream_t stream);

// ------------------------------------------------------------ tmerge.hip
// y (b*t, hw, kt*o) channels_last -> out (b*to, hw, o): sum over the kt taps
// of stride st, p0 frames of zero padding in front
void vfa_temporal_merge(const void* y, void* out, int b, int t, int to,
                        int kt, int st, int p0, int o, long long hw,
                        int relu, int dtype, hipStream_t stream);

// ------------------------------------------------------------ conv2d.hip
// Tile (BM x BN) the conv runs for m = B*OH*OW output pixels and kout
// channels (also bound to Python as conv2d_tile, so a test can pin a shape)
void vfa_conv2d_pick_tile(int m, int kout, int* bm, int* bn);
// x: first element read (the host folds a slice's channel offset in);
// g.pt / g.pl: inline zero-pad applied by the kernel (zp = 1 KiB zero page);
// 0 with pre-padded g.hp / g.wp when the pad was materialized
// ldc: output row stride in elements (= kout normally; larger when the
// epilogue writes a channel slice of a wider NHWC buffer)
void vfa_conv2d_nhwc(const void* x, const void* w, const void* bias,
                     const void* res, const void* zp, void* out,
                     const ConvGeom& g, const ConvAddr& a, int ldc, int act,
                     hipStream_t stream);
// (b, h, w, cin) -> (b, h + pt + pb, w + pl + pr, cout), zeros elsewhere;
// cout % 8 == 0
void vfa_pad2d_nhwc(const void* x, void* out, int b, int h, int w, int cin,
                    int cout, int pt, int pb, int pl, int pr,
                    hipStream_t stream);

// ---------------------------------------------------------- attnpool.hip
// x (b, hw, c) bf16, pos (hw + 1, c) -> t (b, hw + 1, c): mean token first,
// positional embedding added; c % 8 == 0
void vfa_attnpool_tokens(const void* x, const void* pos, void* t, long long b,
                         int hw, int c, hipStream_t stream);
// q (b, heads*64), kv (b, l, 2*heads*64) packed [k | v] -> out (b, heads*64)
void vfa_attention_pool_d64(const void* q, const void* kv, void* out,
                            long long b, int heads, int l, float scale,
                            hipStream_t stream);

}  // extern "C"
