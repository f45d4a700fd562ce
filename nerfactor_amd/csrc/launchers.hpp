// launchers.hpp — every host function of libnfx.so that one translation unit defines and another calls, and that is not
// part of the C-ABI (include/nfx.h): the kernel launchers of the .hip files, their size / plan queries and the option
// lookup.  Each definition includes this header too, so a parameter list that drifts from its declaration does not compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/nfx.h"

namespace nfx::generic { struct Args; struct EmbedArgs; struct BwdArgs; struct WgradArgs; }   // mlp_generic.hpp
namespace nfx::rowsgeom { struct Args; }                                                      // brdf_rows_geom.hpp
namespace nfx::geo { struct Points; }                                                         // nerf_points.hpp

// Host-side description of one weight-gradient GEMM of a batched launch (train.hip; capi_train.cpp fills these).
struct nfx_wgrad_call {
    const void* xt;
    const void* zt;
    int k_in, n_out;
    float* dw;
    float* db;
};

extern "C" {
// ---- capi.cpp: the value of a set option (nfx_set_option), else dflt
int nfx_option_int(const char* key, int dflt);
// ---- brdf_bwd.hip
int nfx_brdf_train_blob_bytes(void);
int nfx_launch_brdf_spec_bwd(const float* xyz, const float* cam, const float* normal, const float* z, int z_dim, const float* lxyz,
                             int n_lights, const void* blob, long long n, const float* dspec, float* d_z, float* d_normal, void* workspace,
                             int max_blocks, hipStream_t st, void* list_ws);
int nfx_brdf_rows_feats(void);
int nfx_launch_brdf_rows(int bwd, const float* z, int z_dim, const float* rusink, long long n, long long rows, const void* blob,
                         const float* dout, float* out_or_dz, void* wsp, long long ld, int max_blocks, hipStream_t st);
// ---- brdf_rows_geom.hip
int nfx_launch_brdf_rows_geom(const nfx::rowsgeom::Args* a, int bwd, hipStream_t st);
// ---- brdf_sphere.hip
int nfx_launch_brdf_sphere(const float* xyz, const float* normal, long long n, const float* cam3, const float* z, int z_dim, int n_iden,
                           const float* lxyz, const float* lweight, int n_lights, const void* blob, float* rgb, int max_blocks,
                           hipStream_t st);
// ---- merl.hip
int nfx_launch_merl_query(const void* table4, const float* rusink, long long n, float* rgb, int* idx, hipStream_t st);
int nfx_launch_merl_sphere(const float* xyz, const float* normal, long long n, const float* cam3, const void* table4, const float* lxyz,
                           const float* lweight, int n_lights, float* rgb, int* idx, hipStream_t st);
// ---- mesh_cast.hip (blob: mesh_bvh.hpp; the counts are the checked header's)
int nfx_launch_mesh_cast(const void* blob, int n_nodes, int n_tris, const float* rayo, const float* rayd, long long n, float* t, int* tri,
                         hipStream_t st);
int nfx_launch_mesh_lvis(const void* blob, int n_nodes, int n_tris, const float* xyz, const float* normal, const float* alpha, long long n,
                         const float* lxyz, int n_lights, float eps, float* lvis, hipStream_t st);
// ---- isosurface.hip (workspace layout and tables: include/nfx.h)
size_t nfx_isosurface_ws_bytes(long long n_pts);
void nfx_isosurface_host_tables(int8_t* tri, int8_t* edge);
int nfx_launch_isosurface_count(const float* field, int nx, int ny, int nz, float iso, void* ws, hipStream_t st);
int nfx_launch_isosurface_emit(const float* field, int nx, int ny, int nz, float iso, const float* origin, const float* spacing,
                               const void* ws, int nv, int nf, float* vertices, int* faces, hipStream_t st);
// ---- mesh_components.hip (label doubles as the parent array; skipped: word 0 of the workspace)
int nfx_launch_mesh_components(const int* faces, long long nf, long long nv, int* label, int* skipped, hipStream_t st);
// ---- image_metrics.hip (cp: channels scored; partial: the workspace, four int64 per block; totals: int64 [batch, 8])
int nfx_launch_image_metrics(const void* a, const void* b, int is_float, int batch, int h, int w, int c, int cp, double max_val,
                             const unsigned char* mask, double* ssim_map, const double* host_weights, long long* totals,
                             long long* partial, hipStream_t st);
// ---- resize.hip (in_type: NFX_RESIZE_*; the tables: include/nfx.h; NFX_EINVAL when an image has more than 2^31 - 1 tiles)
int nfx_launch_resize_antialias(const void* in, int in_type, int batch, int h, int w, int c, float in_scale, const int* first_y,
                                const int* count_y, const float* weights_y, int taps_y, const int* first_x, const int* count_x,
                                const float* weights_x, int taps_x, void* out, int out_uint8, int oh, int ow, hipStream_t st);
// ---- loss.hip
int nfx_launch_pair_loss(int bwd, const nfx_loss_term* terms, int n_terms, const float* alpha, float bg, long long n, float* loss,
                         const float* dloss, hipStream_t st);
// ---- lvis_v2.hip
int nfx_launch_lvis_v2(const float* xyz, long long n, const float* lxyz, int n_lights, const float* pre, const void* blob_main, float* lvis,
                       int ct, int max_blocks, hipStream_t st, const int* out_row, int* nan_flag);
int nfx_launch_brdf_spec_v2(const float* xyz, const float* cam, const float* normal, const float* z, int z_dim, const float* lxyz,
                            int n_lights, const void* blob, long long n, float* spec, int ct, int max_blocks, hipStream_t st);
int nfx_launch_brdf_spec_v3(const float* xyz, const float* cam, const float* normal, const float* z, int z_dim, const float* lxyz,
                            int n_lights, const void* blob, long long n, float* spec, int ct, int geo, int max_blocks, hipStream_t st);
// ---- mlp128.hip
int nfx_launch_mlp128_xyz(const float* xyz, long long n, float xyz_scale, const void* blob, int out_dim, int out_act, float post_scale,
                          float post_bias, float* out, int max_blocks, hipStream_t st);
int nfx_launch_lvis_pre(const float* xyz, long long n, float xyz_scale, const void* blob_pre, float* pre, int max_blocks, hipStream_t st);
int nfx_launch_lvis(const float* xyz, long long n, const float* lxyz, int n_lights, const float* pre, const void* blob_main, float* lvis,
                    int max_blocks, hipStream_t st);
int nfx_launch_brdf_spec(const float* xyz, const float* cam, const float* normal, const float* z, int z_dim, const float* lxyz,
                         int n_lights, const void* blob, long long n, float* spec, int max_blocks, hipStream_t st);
// ---- mlp128_bwd.hip
int nfx_launch_mlp128_bwd(int in_kind, const float* xyz, const float* xyz_dir, long long n, float xyz_scale, const float* lxyz,
                          int n_lights, const void* blob, int out_dim, int out_act, float post_scale, const float* dout, void* wsp,
                          long long ld, int max_blocks, hipStream_t st);
int nfx_mlp128_train_feats(int in_kind);
int nfx_mlp128_train_blob_bytes(int in_kind);
// ---- mlp128_bwd_fused.hip
size_t nfx_mlp128_fused_partial_floats(int in_kind, int grid);
int nfx_mlp128_fused_grid(int in_kind, long long n, int n_lights, int max_blocks);
int nfx_launch_mlp128_bwd_fused(int in_kind, const float* xyz, const float* xyz_dir, long long n, float xyz_scale, const float* lxyz,
                                int n_lights, int n_heads, const void* const* blobs, const int* out_dims, const int* out_acts,
                                const float* post_scales, const float* const* douts, float* partial, int grid, float* const* dk,
                                float* const* db, hipStream_t st);
// ---- mlp128_x3.hip
int nfx_mlp128_x3_weight_bytes(int in_kind);
int nfx_launch_mlp128_x3(int in_kind, const float* xyz, const float* xyz_dir, const float* lxyz, const float* cam, const float* normal,
                         const float* z, int z_dim, long long n, int n_lights, float xyz_scale, const void* blob, int out_dim, int out_act,
                         float post_scale, float post_bias, float* out, int max_blocks, hipStream_t st);
// ---- mlp_generic.hip (nfx_generic_*_m<mode>: one pair per translation unit that includes it, mlp_generic{,_x3,_native}.hip)
int nfx_generic_fwd_m0(const nfx::generic::Args* args, int nw, int grid, int lds, hipStream_t st);
int nfx_generic_fwd_m1(const nfx::generic::Args* args, int nw, int grid, int lds, hipStream_t st);
int nfx_generic_fwd_m2(const nfx::generic::Args* args, int nw, int grid, int lds, hipStream_t st);
int nfx_generic_bwd_m0(const nfx::generic::BwdArgs* ba, const nfx::generic::WgradArgs* wa, int nw, int grid, int lds, hipStream_t st);
int nfx_generic_bwd_m1(const nfx::generic::BwdArgs* ba, const nfx::generic::WgradArgs* wa, int nw, int grid, int lds, hipStream_t st);
int nfx_generic_bwd_m2(const nfx::generic::BwdArgs* ba, const nfx::generic::WgradArgs* wa, int nw, int grid, int lds, hipStream_t st);
int nfx_launch_mlp_generic(const nfx::generic::Args* args, int max_blocks, hipStream_t st);
int nfx_launch_mlp_generic_bwd(const nfx::generic::BwdArgs* ba, const nfx::generic::WgradArgs* wa, int max_blocks, hipStream_t st);
int nfx_launch_split_hilo(void* frags, long long n_frags, hipStream_t st);
int nfx_launch_embed_bwd(const nfx::generic::EmbedArgs* a, const float* d_out, float* dv, hipStream_t st);
int nfx_launch_embed(const nfx::generic::EmbedArgs* a, hipStream_t st);
// ---- nerf_bwd.hip
size_t nfx_nerf_bwd_list_bytes(long long n_pts);
int nfx_launch_nerf_bwd(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples, const void* blob,
                        const float* d_rgbs, void* wsp, long long ld, int max_blocks, hipStream_t st, void* list_ws);
// ---- nerf_fold.hip
int nfx_launch_nerf_fold(const void* blob, void* out, void* ctrl, hipStream_t stream);
// ---- nerf_geom.hip (the gradient launchers take the every-sample and the list form of Points, and refuse the last-sample one)
int nfx_launch_nerf_sigma_grad(const nfx::geo::Points* pts, const void* blob, float* out, int max_blocks, hipStream_t st);
int nfx_launch_select_density(const float* sigma, long long n_pts, float* out, void* list_ws, hipStream_t st);
int nfx_launch_nerf_sigma_geo(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples, const void* blob,
                              float* out, int max_blocks, hipStream_t st);
// ---- nerf_geom_x3.hip
int nfx_launch_nerf_sigma_grad_x3(const nfx::geo::Points* pts, const void* blob, float* out, int max_blocks, hipStream_t st);
int nfx_launch_nerf_sigma_x3(const nfx::geo::Points* pts, const void* blob, float* out, int max_blocks, hipStream_t st);
// ---- nerf_mlp.hip
int nfx_launch_nerf_mlp_bf16(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples, const void* blob,
                             float* out, int variant, int max_blocks, hipStream_t stream);
int nfx_launch_nerf_mlp_bf16_fold(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples, const void* blob,
                                  float* out, int variant, int max_blocks, hipStream_t stream);
// ---- nerf_mlp_v6.hip
int nfx_launch_nerf_mlp_bf16_v6(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples, const void* blob,
                                float* out, int max_blocks, int dma_mode, hipStream_t stream);
int nfx_launch_nerf_mlp_bf16_v6_fold(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples, const void* blob,
                                     float* out, int max_blocks, int dma_mode, unsigned* counter, hipStream_t stream);
// ---- nerf_mlp_x3.hip
int nfx_launch_nerf_mlp_x3(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples, const void* blob,
                           float* out, int max_blocks, hipStream_t stream);
// ---- nerf_sigma_v6.hip
int nfx_launch_nerf_sigma_v6(const float* rayo, const float* rayd, const float* z, long long n_pts, int n_samples, const void* blob,
                             float* out, int max_blocks, hipStream_t stream);
int nfx_launch_nerf_sigma_v6_list(const float* rayo, const float* rayd, const float* z, long long capacity, int n_samples, const void* blob,
                                  float* out, const int* list, const int* count, int max_blocks, hipStream_t stream);
// ---- nerf_sigma_x3_pipe.hip
int nfx_launch_nerf_sigma_x3_pipe(const nfx::geo::Points* pts, const void* blob, float* out, int max_blocks, hipStream_t st);
// ---- occgrid.hip
size_t nfx_occgrid_list_bytes(long long n_pts);
int nfx_launch_occgrid_select(const float* rayo, const float* rayd, const float* z, long long n_rays, int n_samples, const uint32_t* bits,
                              int res, const float* box, const float* bbox, float* out, void* ws, hipStream_t st);
int nfx_launch_occgrid_bake(const float* sigma, int res, int probes, float margin, int dilate, uint32_t* bits, uint32_t* ws,
                            hipStream_t st);
// ---- pack_gather.hip
int nfx_launch_pack_gather(const float* src, const int* map, long long n_words, void* blob, hipStream_t st);
// ---- raymarch.hip
int nfx_launch_l2_normalize3(const float* in, float* out, long long n, float eps, hipStream_t st);
int nfx_launch_gen_z(float near, float far, int n_samples, long long n_rays, int lin_in_disp, const float* u, float* z, hipStream_t st);
int nfx_launch_composite(const float* rgbs, const float* z, const float* rayd, const float* noise, long long n_rays, int S, int white_bg,
                         float* rgb, float* occu, float* depth, float* disp, float* w, hipStream_t st);
int nfx_launch_surface(const float* sigma, const float* z, const float* rayo, const float* rayd, long long n_rays, int S, float occu_thres,
                       int quantize, float* alpha, float* xyz, float* depth, float* occu, hipStream_t st);
int nfx_launch_refine_select(const float* rgbs, const float* z, const float* rayd, long long n_rays, int S, float t_min, float a_lo,
                             float a_hi, float sigma_margin, int dilate, int* list, int* count, hipStream_t st);
int nfx_launch_sample_fine(const float* z, const float* w, long long n_rays, int nc, int nf, const float* u, float* z_all, hipStream_t st);
int nfx_launch_composite_bwd(const float* rgbs, const float* z, const float* rayd, const float* noise, long long n_rays, int n_samples,
                             int white_bg, const float* d_rgb, float* d_rgbs, hipStream_t st);
int nfx_launch_scatter_rows(const float* src, const int* row_of, long long n_all, int d, float* dst, hipStream_t st);
int nfx_launch_zero_rows(float* dst, const int* row_of, long long n_all, int d, hipStream_t st);
int nfx_launch_nonfinite(const float* x, long long n, int* flag, hipStream_t st);
// ---- regularizers.hip
int nfx_launch_l2_normalize_rows(int bwd, const float* x, const float* dy, float* out, long long n, int d, float eps, hipStream_t st);
int nfx_launch_light_smoothness(const float* light, int H, int W, float tv_w, float achro_w, float* loss, float* grad, hipStream_t st);
// ---- selftest.hip
int nfx_launch_selftest_tr16(const float* h, const float* z, float* d, int mode, hipStream_t st);
int nfx_launch_selftest_mfma(const float* a, const float* b, float* d, hipStream_t st);
int nfx_launch_selftest_sincos(const float* in, long long n, int which, float* out, hipStream_t st);
// ---- shade.hip
size_t nfx_shade_olat_lds_bytes(int n_lights);
int nfx_launch_shade(const float* xyz, const float* cam, const float* normal, const float* albedo, const float* rough, const float* spec,
                     float spec_scale, float f0, const float* lvis, const float* lxyz, const float* lareas, const float* lights,
                     long long n, int n_lights, int n_probes, int to_srgb, float* out, hipStream_t st, const int* lvis_row);
int nfx_launch_shade_olat(const float* xyz, const float* cam, const float* normal, const float* albedo, const float* rough,
                          const float* spec, float spec_scale, float f0, const float* lvis, const float* lxyz, const float* lareas,
                          float olat_inten, float ambient, long long n, int n_lights, int to_srgb, float* out, hipStream_t st,
                          const int* lvis_row, const int* out_row, int* nan_flag);
int nfx_launch_dir2rusink(const float* a, const float* b, long long n, float* out, hipStream_t st);
size_t nfx_shade_bwd_lds_bytes(int n_lights, int with_light_grad);
int nfx_launch_shade_bwd(const float* xyz, const float* cam, const float* normal, const float* albedo, const float* rough,
                         const float* spec, float spec_scale, float f0, const float* lvis, const float* lxyz, const float* lareas,
                         const float* light, long long n, int n_lights, int to_srgb, const float* drgb, float* d_albedo, float* d_rough,
                         float* d_spec, float* d_normal, float* d_lvis, float* d_light, void* workspace, hipStream_t st);
// ---- train.hip
int nfx_launch_amsgrad(float* p, const float* g, float* m, float* v, float* vhat, long long n, float lr_t, float b1, float b2, float eps,
                       hipStream_t st);
int nfx_launch_amsgrad_dev(float* p, const float* g, float* m, float* v, float* vhat, long long n, const float* lr_t_dev, float b1,
                           float b2, float eps, hipStream_t st);
size_t nfx_wgrad_partial_bytes(const nfx_wgrad_call* calls, int n_calls, long long rows);
int nfx_launch_wgrad_batch_counted(const nfx_wgrad_call* calls, int n_calls, long long ld, long long rows, void* partial, const int* count,
                                   hipStream_t st);
int nfx_launch_wgrad_batch(const nfx_wgrad_call* calls, int n_calls, long long ld, long long rows, void* partial, hipStream_t st);
void nfx_wgrad_plan_of(const nfx_wgrad_call* calls, int n_calls, long long rows, int* form, long long* slab, int* n_slabs);
int nfx_wgrad_max_calls(void);
int nfx_wgrad_counted_ok(long long rows);
}  // extern "C"
