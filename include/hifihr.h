/*
 * libhifihr.so -- C ABI of the MI355X-native HiFiHR training hot path.
 *
 * The reference (viridityzhu/HiFiHR) has no FFI layer: its hot path is reached through plain Python
 * call sites.  Every entry point below replaces one of those call sites and
 * cites it.  Conventions:
 *   - every function returns 0 on success, a negative HIFIHR_E* code on failure;
 *     hifihr_last_error() returns a thread-local message.  No exceptions cross the ABI.
 *   - pointers named *_d are DEVICE pointers (HBM), *_h are HOST pointers; fp32 unless stated.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  No hidden syncs, no
 *     allocation inside compute calls: the caller owns every buffer; handles own only their tables.
 *   - handles are immutable after create; compute calls are re-entrant on different streams.
 */
#ifndef HIFIHR_H
#define HIFIHR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIFIHR_OK 0
#define HIFIHR_EINVAL (-1)   /* bad argument */
#define HIFIHR_EHIP (-2)     /* HIP runtime error (message has hipGetErrorString) */
#define HIFIHR_ENOMEM (-3)

#define HIFIHR_MANO_NV 778
#define HIFIHR_MANO_NF 1538
#define HIFIHR_MANO_NJ 16

/* 2: every Winograd entry takes the tile edge m under its plain name (the `_m` twins of version 1 are gone) and hifihr_bgemm_describe the batch */
int hifihr_version(void);
const char* hifihr_last_error(void);
/* number of HIP devices visible to the library (<=0: the library cannot be used for compute) */
int hifihr_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * MANO linear-blend skinning.
 * Replaces ManoLayer.__init__/forward   reference utils/my_mano.py:231-313, 315-483
 *          (as configured by MyMANOLayer, utils/my_mano.py:35-36: center_idx=9, flat_hand_mean=False,
 *           side='right', use_pca=True, ncomps=48 => 45 effective PCA coefficients, axis-angle root)
 *          batch_rodrigues/quat2mat      reference utils/manopth/rodrigues_layer.py:43-54,15-40
 *          xyz_from_vertice              reference utils/Freihand_GNN_mano/Freihand_trainer_mano_fullsup.py:175-215
 * Rodrigues keeps the reference's form, angle = || axisang + 1e-8 ||: a rotation vector of exactly 0 (and of exactly pi) is regular, forward
 * and backward; the one singular input is the reference's own, every component exactly -1e-8 (angle 0, 0 / 0): NaN here as in fp32 and
 * float64 PyTorch.
 * All compute entries below: B = 0 is accepted and writes nothing (nothing is launched); B < 0, root_id >= 21 and a NULL among the
 * pointers not marked optional are refused with HIFIHR_EINVAL, nothing launched or written.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hifihr_mano hifihr_mano_t;

/* Tables are host arrays in the layout ManoLayer registers them (my_mano.py:283-313):
 * v_template[778][3], shapedirs[778][3][10], posedirs[778][3][135], j_regressor[16][778] (dense),
 * weights[778][16], hands_components[45][45] (row k = component k), hands_mean[45]. */
int hifihr_mano_create(hifihr_mano_t** out, const float* v_template_h, const float* shapedirs_h,
                       const float* posedirs_h, const float* j_regressor_h, const float* weights_h,
                       const float* hands_components_h, const float* hands_mean_h);
int hifihr_mano_destroy(hifihr_mano_t* h);

/* ManoLayer.forward(th_pose_coeffs=pose[B][48], th_betas=beta[B][10]) -> th_verts[B][778][3],
 * th_jtr[B][21][3] (both centred on joint 9; th_trans==0 branch, my_mano.py:471-475).
 * saved_vposed_d[B][778][3] receives v_posed (my_mano.py:392) for the backward pass; may be NULL when
 * no backward follows. */
int hifihr_mano_lbs_fwd(const hifihr_mano_t* h, const float* pose_d, const float* beta_d, int B,
                        float* verts_d, float* jtr_d, float* saved_vposed_d, void* stream);

/* Gradient of the above: gverts[B][778][3], gjtr[B][21][3] (either may be NULL = zero) ->
 * gpose[B][48], gbeta[B][10] (overwritten).  Deterministic (no float atomics).  jtr_d of the forward may be NULL too. */
int hifihr_mano_lbs_bwd(const hifihr_mano_t* h, const float* pose_d, const float* beta_d,
                        const float* saved_vposed_d, const float* gverts_d, const float* gjtr_d, int B,
                        float* gpose_d, float* gbeta_d, void* stream);

/* xyz_from_vertice(verts).permute(1,0,2) followed by the root-relative step of Model.forward
 * (reference models_res_nimble.py:153,160-166, training branch):
 *   joints21 = regress(verts); root = joints21[:, root_id]; joints_rel = joints21 - root;
 *   verts_rel = verts - root.   root_id < 0 skips the subtraction (root_d then receives zeros).
 * Outputs joints_rel_d[B][21][3], verts_rel_d[B][778][3] (may alias verts_d), root_d[B][3]. */
int hifihr_mano_joints_fwd(const hifihr_mano_t* h, const float* verts_d, int B, int root_id,
                           float* joints_rel_d, float* verts_rel_d, float* root_d, void* stream);
/* Gradient: gjoints_rel[B][21][3], gverts_rel[B][778][3], groot[B][3] (any may be NULL) ->
 * gverts[B][778][3] (overwritten). */
int hifihr_mano_joints_bwd(const hifihr_mano_t* h, const float* gjoints_rel_d, const float* gverts_rel_d,
                           const float* groot_d, int B, int root_id, float* gverts_d, void* stream);

/* The two steps above as ONE call per direction (round 5), with the mesh offset `skin_meshes.offset_verts_(-pred_root);
 * .offset_verts_(root_xyz)` that precedes the renderer folded in
 * (reference utils/my_mano.py:315-483; Freihand_trainer_mano_fullsup.py:175-215; models_res_nimble.py:153,160-166,203-205):
 *   verts = layer(pose, beta); joints21 = regress(verts); root = joints21[:, root_id];
 *   joints_rel = joints21 - root; verts_rel = verts - root; verts_cam = verts_rel + root_xyz.
 * Forward: two launches (the layer; regression + offsets); backward: ONE launch (the regression's backward is the head of the layer's).
 * verts_d[B][778][3] receives the layer's (absolute, centred) vertices.  root_xyz_d[B][3] / verts_cam_d / root_d may be NULL.
 * saved_vposed_d as in hifihr_mano_lbs_fwd.  Results are bit-identical to the two-call form. */
int hifihr_mano_full_fwd(const hifihr_mano_t* h, const float* pose_d, const float* beta_d, int B, int root_id,
                         const float* root_xyz_d, float* verts_d, float* joints_rel_d, float* verts_rel_d, float* verts_cam_d,
                         float* root_d, float* saved_vposed_d, void* stream);
/* Gradient: gjoints_rel[B][21][3], gverts_rel[B][778][3], gverts_cam[B][778][3], groot[B][3] (any may be NULL = zero) ->
 * gpose[B][48], gbeta[B][10] (overwritten).  gpose_add_d[B][48] / gbeta_add_d[B][10] (may be NULL) are ADDED to the results: the
 * gradient that reaches pose / beta through their other consumer (the mpose / mshape terms of losses.py:283-284), so that the sum
 * costs no launch of its own.  Deterministic (no float atomics). */
int hifihr_mano_full_bwd(const hifihr_mano_t* h, const float* pose_d, const float* beta_d, const float* saved_vposed_d,
                         const float* gjoints_rel_d, const float* gverts_rel_d, const float* gverts_cam_d,
                         const float* groot_d, const float* gpose_add_d, const float* gbeta_add_d, int B, int root_id,
                         float* gpose_d, float* gbeta_d, void* stream);

/* Test-time fit of the MANO parameters to 2-D / 3-D keypoints (the reference's mano_fitting, utils/traineval_util.py:505-595, on the
 * live layer's parametrisation) in ONE launch: one workgroup per hand, every iteration inside the kernel, the hands independent.
 * In / out (updated in place): pose_d[B][48] (3 root axis-angle + 45 PCA coefficients), beta_d[B][10], root_d[B][3] (absolute position of
 * the root joint, in the unit of the vertices).  In: K_d[B][3][3], kp2d_d[B][21][2] in pixels, conf2d_d[B][21]; kp3d_d[B][21][3] with
 * conf3d_d[B][21] (both NULL: no 3-D term); prior_lo_d / prior_hi_d / prior_w_d [48] (all NULL: no pose prior); lr_d[iters] (device);
 * weights6_host = (w2d, wbone, w3d, wprior, wshape, wpca) and lr_mult4_host = (root rotation, pose coefficients, shape, root position),
 * host memory.  Out: trace_d[B][iters + 1][8], grad0_d[B][61] (may be NULL), done_d[B].
 * One iteration, in this order:
 *   1. the layer (hifihr_mano_lbs_fwd without its centring), joints21 = regress(verts), J_rel = joints21 - joints21[root_id];
 *   2. X = J_rel + root, p = K X, uv = p_xy / p_z.  A joint with X_z <= 1e-4 is left out of the two 2-D terms for this iteration (its
 *      confidence counts as 0); K is expected to be a pinhole matrix with last row (0, 0, 1), so that p_z = X_z;
 *   3. E = w2d e2d + wbone ebone + w3d e3d + wprior eprior + wshape eshape + wpca epca, per hand:
 *        e2d    = sum_j c_j^2 rho(d_j) / sum_j c_j^2, d = |uv - kp2d|, rho and its d = 0 corner as hifihr_open2d_terms_* (no joint weights:
 *                 a caller folds them into c); sum c^2 = 0: exactly 0 with a zero gradient
 *        ebone  = mean over the 20 bones of |vn - von|^2 c_parent c_child, unit vectors v / (|v| + 1e-4), corners as hifihr_open2d_terms_*
 *        e3d    = sum_j c3_j |J_rel_j - kp3d_j|^2 / sum_j c3_j (sum c3 = 0: exactly 0)
 *        eprior = (1/48) sum_i w_i (max(fp_i - hi_i, 0) + max(lo_i - fp_i, 0)) on the full axis-angle pose fp = (pose[0:3], mean + PCA);
 *                 strict comparisons (the reference's torch.where, utils/losses_util.py:139-215): the slope is 0 at a bound
 *        eshape = mean beta^2, epca = mean pose[3:48]^2
 *      trace[b][i] = (E, e2d, ebone, e3d, eprior, eshape, epca, mean d_j over the joints with c_j > 0 that were not left out), taken at
 *      the parameters BEFORE update i; row `iters` is taken at the result;
 *   4. the hand-derived gradient through projection, root-relative step, joint regression, tips and the layer (grad0 = dE / d(pose, beta,
 *      root) of iteration 0);
 *   5. Adam in torch's form, beta = (0.9, 0.999), eps = 1e-8, step t = i + 1: m = m + 0.1 (g - m), v = 0.999 v + 0.001 g^2,
 *      p -= lr_i mult_g / (1 - 0.9^t) x m / (sqrt(v) / sqrt(1 - 0.999^t) + eps); the moments start at 0 and are KEPT across iterations.
 *      A DELIBERATE departure: the reference builds a new optimiser every iteration, which resets its moments (each step is then
 *      lr x sign(g)); that is not reproduced.  A group whose multiplier is 0 is not touched: its bits stay.
 * Decided behaviours:
 *   - iters == 0 evaluates only (trace row 0, grad0): the parameters keep the bits they came with.
 *   - a hand whose E, gradient or updated parameters turn non-finite at iteration i stops there: its parameters are those before update i
 *     (the inputs for i = 0), done[b] = i, trace row i holds what was evaluated and the rows after it are 0.  Otherwise done[b] = iters.
 *     The other hands are unaffected.  A non-finite keypoint counts even at confidence 0.
 *   - deterministic: the same bits on a second call, and for a hand whatever the batch around it (fixed summation orders, no atomics).
 * Nothing is allocated or synchronised; the call can be captured in a graph.
 * Refused (HIFIHR_EINVAL, nothing launched or written): B <= 0, iters < 0, root_id outside 0 .. 20, a NULL handle / pose / beta / root /
 * K / kp2d / conf2d / weights / lr_mult / trace / done, NULL lr with iters > 0, kp3d without conf3d or the reverse, a prior table without
 * the other two, a weight or multiplier that is negative or not finite. */
int hifihr_mano_fit(const hifihr_mano_t* h, float* pose_d, float* beta_d, float* root_d, const float* K_d, const float* kp2d_d,
                    const float* conf2d_d, const float* kp3d_d, const float* conf3d_d, const float* prior_lo_d, const float* prior_hi_d,
                    const float* prior_w_d, const float* lr_d, int iters, const float* weights6_host, const float* lr_mult4_host,
                    int root_id, int B, float* trace_d, float* grad0_d, int32_t* done_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Generic linear-blend skinning (any mesh size / kinematic tree): the NIMBLE-shaped hand layer.
 * Replaces the skinning step of  self.hand_layer(hand_params, handle_collision=False)  when `hand_model: "nimble"`
 *          (reference models_res_nimble.py:56-57,133-142; MyNIMBLELayer itself is an un-vendored submodule -- SURVEY.md section 8 A9 --
 *          so the formulation is the MANO one of utils/my_mano.py:386-451 without pose-corrective blend shapes:
 *          v_shaped = v_template + shapedirs . beta;  J = j_regressor . v_shaped;  R = Rodrigues(theta);
 *          global transforms down `parents`;  v = sum_j weights[v][j] (G_j [v_shaped; 1] - G_j [J_j; 0])).
 * ---------------------------------------------------------------------------------------------- */
typedef struct hifihr_lbs hifihr_lbs_t;

/* Host tables: v_template[V][3], shapedirs[V][3][S], j_regressor[J][V] (dense), weights[V][J] (dense; at most 8 non-zeros per
 * row, kept exactly), parents[J] (parents[0] = -1, parents[j] < j).  1 <= J <= 32, 0 <= S <= 32. */
int hifihr_lbs_create(hifihr_lbs_t** out, int V, int J, int S, const float* v_template_h, const float* shapedirs_h,
                      const float* j_regressor_h, const float* weights_h, const int* parents_h);
int hifihr_lbs_destroy(hifihr_lbs_t* h);

/* theta[B][J][3] (axis-angle per joint, joint 0 = global rotation), beta[B][S] -> verts[B][V][3], joints[B][J][3] (posed joint
 * positions; may be NULL).  No centring. */
int hifihr_lbs_fwd(const hifihr_lbs_t* h, const float* theta_d, const float* beta_d, int B, float* verts_d, float* joints_d, void* stream);

/* Gradient: gverts[B][V][3], gjoints[B][J][3] (may be NULL = zero) -> gtheta[B][J][3] (overwritten), gbeta[B][S] (ACCUMULATED: the
 * caller passes it zeroed).  scratch[B][J][12] must be zero on entry; it is left holding d(loss)/d(A_j).  Sums over vertices use float
 * atomics: results vary in the last bits from run to run.
 * Accumulated / overwritten: gtheta is OVERWRITTEN; gbeta is ACCUMULATED onto whatever it holds; scratch is ACCUMULATED onto its zeros and
 * comes back as d(sum gverts . verts) / d(A_j) = sum_v weights[v][j] gverts_v [v_shaped_v; 1]^T, 3 x 4 row-major (the gjoints part of the
 * gradient goes down the chain without passing through it).  B = 0: accepted, nothing written; B < 0 or a NULL among theta, gverts,
 * scratch, gtheta, verts (and beta / gbeta when S > 0): HIFIHR_EINVAL. */
int hifihr_lbs_bwd(const hifihr_lbs_t* h, const float* theta_d, const float* beta_d, const float* gverts_d, const float* gjoints_d,
                   int B, float* scratch_zeroed_d, float* gtheta_d, float* gbeta_zeroed_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Hard rasteriser + Phong shader + anti-aliasing resolve.
 * Replaces  rendered = self.renderer_p3d(skin_meshes, cameras=cameras, lights=lighting)
 *           rendered = F.avg_pool2d(rendered.permute(0,3,1,2), aa, aa)      reference models_res_nimble.py:208-211
 * with the renderer built as in models_res_nimble.py:70-96 (MeshRasterizer(image_size*aa, blur 0, 1 face per
 * pixel) + HardPhongShader) and cameras/lights as in :184-190.  PyTorch3D semantics are restated in
 * oracle/raster_oracle.c and oracle/render_oracle.py (parity unpinned at that third-party boundary).
 * Meshes share one topology (faces) across the batch, as MyMANOLayer/MyNIMBLELayer produce them.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hifihr_renderer hifihr_renderer_t;

/* Refused / accepted, for every entry of this block (tests/test_hostsim_render_contract.py walks each of them):
 *   Refused (HIFIHR_EINVAL, nothing launched, nothing written): a NULL handle or a NULL among the pointers an entry lists -- every one of
 *   them except gvcolors_d of render_bwd and gmaps_acc_d of render_bwd_uv (NULL = that gradient is not wanted) and the two reserved texel
 *   scratch arguments; B < 0; TH < 1 or TW < 1; render_fwd_uv / render_bwd_uv on a renderer without UV tables (before a successful
 *   hifihr_renderer_set_uv).  hifihr_renderer_create: V, F or image_size <= 0, image_size > 720, aa outside 1 .. 3, a face index outside
 *   0 .. V - 1, a NULL among out, faces_h and the four colour pointers (*out is left as it was).  hifihr_renderer_set_uv: n_uv <= 0, an
 *   index outside 0 .. n_uv - 1, a NULL pointer (the renderer keeps the tables it had).  hifihr_renderer_set_light_mode: a mode other than 0, 1.
 *   Accepted: B == 0 is a no-op -- nothing launched, no output and no byte of the workspace touched.  hifihr_render_workspace_bytes(NULL, .)
 *   and (h, B < 0) return 0; the size never decreases with B.  hifihr_render_uv_scratch_bytes is 0.  hifihr_renderer_destroy(NULL) does nothing.
 *   The image-size limit: image_size <= 720.  Up to 512 the forward runs persistent workgroups on a queue whose item code holds 64 x 64
 *   tiles of 8 pixels; above it one workgroup per tile, and the binning kernel's 2 ceil(image_size / 8)^2 ints of dynamic LDS must fit the
 *   64 KiB a launch may request without a function attribute: 90 x 90 tiles (csrc/render.hip, next to f3_supported).
 *   Precondition, NOT checked: every vertex is finite and none has Z == 0 (the projection divides by Z).  Vertices behind the camera plane
 *   (Z < 0) are inside the contract: a face that straddles the plane is rasterised per sample (pz >= 0), one wholly behind it is dropped.
 *   A NaN, an Inf or a zero Z in verts_d gives unspecified pixels and gradients (never an out-of-range access: tile and pixel ranges come
 *   from comparisons against the grid, a texel index from a coordinate clamped to the map first; no unclamped float becomes an index).
 *   A pixel without a covered sample holds the sum of aa^2 background samples over aa^2 (the background colour to rounding; exactly it for
 *   colours whose multiples are exact, 1.0 among them); alpha is exactly hits / aa^2. */

/* faces_h[F][3] int32 (host); image_size = output edge H (224; 1 .. 720), aa = samples per pixel edge (3; 1..3 supported);
 * ambient3 = materials.ambient * lights.ambient, mat_diffuse3 = materials.diffuse,
 * specular3 = materials.specular * lights.specular, background3 = BlendParams.background_color. */
int hifihr_renderer_create(hifihr_renderer_t** out, const int32_t* faces_h, int V, int F, int image_size, int aa,
                           const float* ambient3, const float* mat_diffuse3, const float* specular3, float shininess,
                           const float* background3);
/* point_lights = 1: PointLights instead of DirectionalLights (the reference's light_estimation = false branch,
 * models_res_nimble.py:191-198): light_dir_d[B][3] of render_fwd / bwd is then the light's LOCATION, the direction of a sample is
 * location - point (normalised); the location gets no gradient (glight_dir_d comes back zero). */
int hifihr_renderer_set_light_mode(hifihr_renderer_t* h, int point_lights);
int hifihr_renderer_destroy(hifihr_renderer_t* h);
/* bytes of scratch the caller must pass to render_fwd/bwd for batch B; the SAME buffer, untouched in between,
 * must be passed to the backward call of a forward call (it carries the packed per-vertex records). */
size_t hifihr_render_workspace_bytes(const hifihr_renderer_t* h, int B);

/* verts_d[B][V][3] view-space vertices (R = I, T = 0); vcolors_d per-vertex RGB ([B][V][3] when vcolors_batched,
 * else [V][3] shared); cam_d[B][4] = (fx, fy, px, py) exactly as handed to PerspectiveCameras (i.e. the
 * NEGATED ndc focal lengths, models_res_nimble.py:184-186); light_color_d[B][3] = DirectionalLights.diffuse_color,
 * light_dir_d[B][3] = DirectionalLights.direction (un-normalised).
 * Outputs: rgba_d[B][4][H][H] (NCHW, after the aa x aa average pool; channel 3 = coverage),
 *          face_id_d[B][H*aa][H*aa] int32 = pix_to_face minus the b*F packing offset (-1 = background). */
int hifihr_render_fwd(const hifihr_renderer_t* h, const float* verts_d, const float* vcolors_d, int vcolors_batched,
                      const float* cam_d, const float* light_color_d, const float* light_dir_d, int B, float* rgba_d,
                      int32_t* face_id_d, void* workspace_d, void* stream);

/* grad_rgba_d[B][4][H][H] (the coverage channel carries no gradient, as in the reference: SURVEY.md F7; the differentiable
 * coverage is hifihr_soft_sil_fwd below) ->
 * gverts_d[B][V][3], gvcolors_d[B][V][3] (may be NULL; per image also when the forward's colours were shared), glight_color_d[B][3],
 * glight_dir_d[B][3]; all overwritten.
 * Uses float atomics: results are reproducible to rounding, not bitwise. */
int hifihr_render_bwd(const hifihr_renderer_t* h, const float* verts_d, const float* cam_d, const float* light_color_d,
                      const float* light_dir_d, const int32_t* face_id_d, const float* grad_rgba_d, int B,
                      float* gverts_d, float* gvcolors_d, float* glight_color_d, float* glight_dir_d, void* workspace_d,
                      void* stream);
/* TexturesUV mode (PyTorch3D renderer/mesh/textures.py TexturesUV.sample_textures [recalled]; the reference hands NIMBLE's texture image to
 * the renderer this way, models_res_nimble.py:203-208): per sample uv = sum_k bary_k * verts_uvs[faces_uvs[f][k]] with the rasteriser's
 * perspective-corrected barycentrics, texel = grid_sample(flip(maps, vertical), 2 uv - 1, bilinear, align_corners = True, border padding),
 * shaded like a vertex colour -- inside the fused tile kernels' per-sample shading (a template flag of theirs); the backward returns
 * d loss / d maps (float atomics into gmaps_acc_d, which the caller zeroes) and d loss / d verts including the path through uv.
 *   hifihr_renderer_set_uv(h, faces_uvs_h[F][3], verts_uvs_h[n_uv][2], n_uv)   once per renderer
 *   maps_d[B][TH][TW][3]; texels_scratch_d / gtexels_scratch_d: reserved, pass NULL (hifihr_render_uv_scratch_bytes returns 0) */
int hifihr_renderer_set_uv(hifihr_renderer_t* h, const int32_t* faces_uvs_h, const float* verts_uvs_h, int n_uv);
size_t hifihr_render_uv_scratch_bytes(const hifihr_renderer_t* h, int B);
int hifihr_render_fwd_uv(const hifihr_renderer_t* h, const float* verts_d, const float* maps_d, int TH, int TW, const float* cam_d,
                         const float* light_color_d, const float* light_dir_d, int B, float* rgba_d, int32_t* face_id_d,
                         float* texels_scratch_d, void* ws_d, void* stream);
int hifihr_render_bwd_uv(const hifihr_renderer_t* h, const float* verts_d, const float* maps_d, int TH, int TW, const float* cam_d,
                         const float* light_color_d, const float* light_dir_d, const int32_t* face_id_d, const float* grad_rgba_d, int B,
                         const float* texels_scratch_d, float* gtexels_scratch_d, float* gverts_d, float* gmaps_acc_d,
                         float* glight_color_d, float* glight_dir_d, void* ws_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Soft silhouette (csrc/soft_sil.hip): a differentiable coverage of the mesh at the OUTPUT resolution, next to the hard renderer whose
 * coverage channel carries no gradient.  Semantics of PyTorch3D's rasterize_meshes(blur_radius > 0) + sigmoid_alpha_blend
 * (SoftSilhouetteShader) [recalled: parity is unpinned, like the rest of that boundary].  The entries reuse the renderer handle's faces, V,
 * F and image_size H; aa is ignored (one sample per pixel centre).  Per image b and pixel (yi, xi):
 *   vertices    xn = (X fx + Z px) / Z, yn = (Y fy + Z py) / Z with cam_d[B][4] = (fx, fy, px, py) as for hifihr_render_fwd
 *   centre      (pix_to_ndc(H - 1 - xi, H), pix_to_ndc(H - 1 - yi, H))
 *   per face    area = edge_fn(v2, v0, v1); inside = the three edge functions over area are all > 0; dist = min over the three edges of
 *               the SQUARED distance from the centre to the segment (t clamped to [0, 1]); d = inside ? -dist : dist
 *   a face participates iff its three vertices have Z > 0, |area| > 1e-8 and (inside || dist < blur_radius) -- blur_radius is compared
 *               with the squared distance, as in PyTorch3D
 *   S = sum over participating faces, in face-index order, of softplus(-d / sigma);   alpha = 1 - exp(-S)
 * (= 1 - prod (1 - sigmoid(-d_f / sigma)); a pixel without a participating face is exactly 0).  Defaults of the Python surface:
 * sigma = 1e-4, blur_radius = log(1 / 1e-4 - 1) sigma.
 * Two departures from PyTorch3D: no faces_per_pixel cap (equal whenever K >= the number of participating faces); a face with a vertex at or
 * behind the camera plane (Z <= 0) is left out (PyTorch3D projects such a vertex through the division).
 * Gradient: to verts_d only (cam_d gets none, as in the renderer's Python wrapper); participation, inside, the nearest edge and the clamp
 * are piecewise constant choices.
 *
 * Refused (HIFIHR_EINVAL, nothing launched, nothing written): a NULL handle or pointer; B < 0; sigma not finite or <= 0; blur_radius not
 *   finite or < 0; the loss entries: HW <= 0, mask_i64 outside {0, 1}, and hifihr_soft_sil_loss_bwd B > 65535.
 * Accepted: B == 0 is a no-op (nothing launched, nothing written).  hifihr_soft_sil_workspace_bytes(NULL, .) and (h, B < 0) return 0; the
 *   size never decreases with B.
 * Precondition, NOT checked (as for the renderer): every vertex is finite and none has Z == 0.  A NaN, an Inf or a zero Z gives
 *   unspecified pixels and gradients, never an out-of-range access: every index comes from the face table or from integer arithmetic on
 *   the grid, no float becomes an index.
 * Overwritten / accumulated: hifihr_soft_sil_fwd writes EVERY element of alpha_d[B][H][H] and neglog_d[B][H][H] (= S; the backward reads
 *   S because 1 - alpha has no precision left near full coverage).  hifihr_soft_sil_bwd OVERWRITES gverts_d[B][V][3] (a vertex no
 *   participating face references gets 0); it zeroes its NDC-gradient accumulators inside ws_d itself and depends on nothing a forward
 *   left there, so any ws_d of hifihr_soft_sil_workspace_bytes(h, B) bytes serves either call.  Pixels whose galpha_d is 0 or whose
 *   exp(-S) is 0 are skipped.
 * Repeatable: alpha_d and neglog_d have the same bits on every call (faces are listed per tile in face order by a ballot prefix, no raced
 *   counter).  gverts_d is summed with float atomics (one per component, face corner and tile, after an on-chip sum over the tile's
 *   pixels): reproducible to rounding, not bitwise -- as for hifihr_render_bwd.
 * ws_d: hifihr_soft_sil_workspace_bytes(h, B) bytes, 16-byte aligned (it is written as float4 records; NOT checked).
 * No allocation and no synchronisation inside: the entries can be captured into a hipGraph. */
size_t hifihr_soft_sil_workspace_bytes(const hifihr_renderer_t* h, int B);
int hifihr_soft_sil_fwd(const hifihr_renderer_t* h, const float* verts_d, const float* cam_d, int B, float sigma, float blur_radius,
                        float* alpha_d, float* neglog_d, void* ws_d, void* stream);
int hifihr_soft_sil_bwd(const hifihr_renderer_t* h, const float* verts_d, const float* cam_d, const float* neglog_d, const float* galpha_d,
                        int B, float sigma, float blur_radius, float* gverts_d, void* ws_d, void* stream);
/* The two losses of the soft silhouette in one kernel pair.  alpha_d[B][HW]; mask_d[B][HW] = segms_gt, float32 (mask_i64 = 0) or int64
 * (mask_i64 = 1), M = its value as float.  Per image, in a fixed order and in fp64, one workgroup and no atomics:
 *   sums_d[B][3] = (sum |A - M|, I = sum A M, sum (A + M));
 * a finish step writes out_d[2] = (lam_sil mean |A - M|, lam_iou (1 - mean_b I_b / U_b)), U_b = sum (A + M) - I_b: F.l1_loss and the
 * formula of hifihr_amd.losses.iou, with NO epsilon -- an image with U_b = 0 (empty mask, zero alpha) gives NaN, exactly as `iou` does.
 * A term whose weight is exactly 0 is written as 0 (and gets no gradient) whatever its value would be.  out_d and sums_d are overwritten
 * and have the same bits on every call.  hifihr_soft_sil_loss_bwd: one elementwise launch that OVERWRITES galpha_d[B][HW] from the two
 * upstream scalars gout_d[2] and sums_d (the mask gets no gradient; d|A - M| / dA = 0 where A == M). */
int hifihr_soft_sil_loss_fwd(const float* alpha_d, const void* mask_d, int mask_i64, int B, int HW, float lam_sil, float lam_iou,
                             double* sums_d, float* out_d, void* stream);
int hifihr_soft_sil_loss_bwd(const float* alpha_d, const void* mask_d, int mask_i64, const double* sums_d, const float* gout_d, int B, int HW,
                             float lam_sil, float lam_iou, float* galpha_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth map (csrc/depth.hip): the depth image of the hard render, with a backward pass to the vertices, and a masked depth loss.  The
 * rasteriser already finds every sample's nearest face and its perspective-correct depth; only face_id leaves it.  These entries turn
 * that face_id into a depth map in one pass, without a second rasterisation.  They work on the renderer handle's faces, V, F, image_size
 * H and aa; S = H aa is the edge of the sample grid.
 *
 * Depth map.  For image b and output pixel (y, x), over the aa x aa samples of that pixel in face_id_d[B][S][S] as hifihr_render_fwd or
 * hifihr_render_fwd_uv wrote it for the SAME verts_d and cam_d:
 *   a sample with face_id >= 0 is covered;
 *   its z is the *pz of sample_face() in csrc/render_math.h for that face at that sample centre: the same fp32 expressions in the same
 *     order that the rasteriser and oracle/raster_oracle.c use, built with -ffp-contract=off -- vertices xn = (X fx + Z px) / Z,
 *     yn = (Y fy + Z py) / Z; divided barycentrics w_i = e_i / (area + 1e-8); perspective correction t0 = w0 z1 z2, t1 = z0 w1 z2,
 *     t2 = z0 z1 w2, b_i = t_i / max(t0 + t1 + t2, 1e-8); pz = b0 z0 + b1 z1 + b2 z2.  This is PyTorch3D's fragments.zbuf under
 *     perspective_correct = True [recalled; parity unpinned, like the rest of that boundary];
 *   hits = the number of covered samples; depth_d[b][y][x] = the fp32 sum of z over the covered samples in row-major sample order,
 *     divided by hits (one division), and exactly 0 when hits == 0; hits_d[b][y][x] = hits as int32.
 * At aa = 1 the depth of a covered pixel therefore has the bits of the rasteriser's own zbuf.
 * The background never enters the average.  This departs from the reference's avg_pool2d of rgba on purpose: there the background is a
 * colour, whereas a pooled zbuf with a -1 background would mean nothing.
 * A face_id outside 0 .. F - 1, or one whose sample sample_face() rejects (neither can come from the renderer for these inputs), counts as
 * not covered: no index is formed from it.
 *
 * Depth gradient (hifihr_render_depth_bwd).  To verts_d only; cam_d gets none, as in the renderer's Python wrapper.  face_id, the
 * max(., 1e-8) clamp of the denominator, the rasteriser's pz >= 0 / b_i > 0 tests and hits are piecewise constant choices (where the
 * denominator clamps it carries no gradient).  A covered sample receives gdepth / hits; the gradient flows through z0 .. z2 directly
 * and through the NDC coordinates xn, yn of the three corners.  gverts_d[B][V][3] is OVERWRITTEN; a vertex that no covered sample
 * references gets exactly 0.  Pixels whose gdepth_d is 0 or whose hits_d is <= 0 are skipped.
 * The form built is the atomic one: one wave per tile of 8 x 8 output pixels sums each face's nine components (NDC x, y and Z of its
 * three corners) over the tile on chip and issues ONE float atomic per component, corner and tile into the accumulator float[B][V][3]
 * inside ws_d, which the entry zeroes itself (any ws_d of hifihr_render_depth_workspace_bytes(h, B) bytes, 16-byte aligned, serves); a
 * per-vertex pass applies the projection's chain rule.  depth_d and hits_d have the same bits on every call; gverts_d is reproducible
 * to rounding, NOT bitwise -- as for hifihr_render_bwd.
 *
 * Loss (hifihr_depth_loss_fwd / _bwd).  d = depth_d[B][HW], hits_d[B][HW], the target D = target_d[B][HW] in fp32 where 0 (or less)
 * means no measurement, an optional mask M = mask_d[B][HW], float32 (mask_i64 = 0) or int64 (mask_i64 = 1) as for
 * hifihr_soft_sil_loss_fwd, NULL = all ones, and trunc >= 0.  A pixel is valid iff hits > 0 and D > 0 and M != 0 and
 * (trunc == 0 or |d - D| <= trunc), with d - D taken in fp64 (exact).  Per image, one workgroup, a fixed order, fp64, no atomics:
 *   sums_d[B][2] = (sum over the valid pixels of |d - D|, their count);
 * a finish step writes out_d[1] = lam * sum_b sum_b / max(sum_b count_b, 1), the mean |d - D| over the valid pixels of the batch in the
 * inputs' unit.  A batch without a valid pixel gives exactly 0 and a zero gradient, not NaN: frames without usable depth are ordinary in
 * a mixed batch, and there is no reference formula to reproduce (the reference declares lambda_depth and never computes the term).
 * sums_d and out_d are overwritten and have the same bits on every call.  hifihr_depth_loss_bwd is one elementwise launch that
 * OVERWRITES gdepth_d[B][HW]: gout_d[0] * lam * sign(d - D) / max(sum count, 1) on the valid pixels, 0 on all others and where d == D;
 * validity is treated as constant; the target and the mask get no gradient.
 *
 * Refused (HIFIHR_EINVAL, nothing launched, nothing written): a NULL handle or pointer other than mask_d; B < 0; the loss entries also
 *   HW <= 0, lam or trunc not finite, trunc < 0, mask_i64 outside {0, 1}, and hifihr_depth_loss_bwd B > 65535.
 * Accepted: B == 0 is a no-op.  hifihr_render_depth_workspace_bytes(NULL, .) and (h, B < 0) return 0; the size never decreases with B.
 * Precondition, NOT checked (as for the renderer): every vertex is finite and none has Z == 0.
 * No allocation and no synchronisation inside: the entries can be captured into a hipGraph. */
size_t hifihr_render_depth_workspace_bytes(const hifihr_renderer_t* h, int B);
int hifihr_render_depth_fwd(const hifihr_renderer_t* h, const float* verts_d, const float* cam_d, const int32_t* face_id_d, int B,
                            float* depth_d, int32_t* hits_d, void* stream);
int hifihr_render_depth_bwd(const hifihr_renderer_t* h, const float* verts_d, const float* cam_d, const int32_t* face_id_d,
                            const float* gdepth_d, const int32_t* hits_d, int B, float* gverts_d, void* ws_d, void* stream);
int hifihr_depth_loss_fwd(const float* depth_d, const int32_t* hits_d, const float* target_d, const void* mask_d, int mask_i64, int B, int HW,
                          float lam, float trunc, double* sums_d, float* out_d, void* stream);
int hifihr_depth_loss_bwd(const float* depth_d, const int32_t* hits_d, const float* target_d, const void* mask_d, int mask_i64,
                          const double* sums_d, const float* gout_d, int B, int HW, float lam, float trunc, float* gdepth_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh regularisers (csrc/mesh_reg.hip): `triangle` and `normal_consistency` in one kernel pair.
 * `triangle` replaces reference losses.py:421-429, lambda_laplacian * mesh_laplacian_smoothing(Meshes(verts, faces), method="uniform");
 * `normal_consistency` is PyTorch3D's mesh_normal_consistency, which the reference does not use.  Both PyTorch3D functions are [recalled]:
 * parity with PyTorch3D is unpinned, the kernels are held to the definitions below (tests/mesh_reg_ref.py restates them in float64).
 *
 * Topology, built once on the host from faces[F][3] and V:
 *   edges    the unique unordered vertex pairs of the faces; E = their count
 *   N(i)     the distinct neighbours of vertex i in ascending order; deg(i) = |N(i)|
 *   quads    for every edge (v0 < v1): the opposite vertex of each face that contains the edge, in ascending face order; every unordered
 *            pair (a, b) of that list, a from the lower-indexed face, is one record (v0, v1, a, b); Q = the record count.  A boundary edge
 *            gives no record, an edge shared by three faces gives three.  Records are ordered by (v0, v1), then by the two faces.
 * triangle, for verts[B][V][3]:
 *   d_i = (1 / deg(i)) sum over j in N(i) of v_j  -  v_i;   deg(i) = 0: d_i = -v_i (PyTorch3D's -1 diagonal on every row [recalled])
 *   lap = (1 / (B V)) sum_b sum_i ||d_i||_2;   out[0] = lam_lap lap;   the subgradient at d_i = 0 is 0 (as torch.norm's)
 * normal_consistency, per quad record:
 *   e = v1 - v0, n0 = e x (a - v0), n1 = -(e x (b - v0)), cos = n0 . n1 / (max(||n0||, 1e-8) max(||n1||, 1e-8))
 *   nc = (1 / (B Q)) sum_b sum_q (1 - cos), 0 when Q = 0;   out[1] = lam_nc nc;   the value does not depend on face winding.
 *   A record with a norm at or below the clamp contributes 1 - cos to the value and NO gradient (a stated piecewise choice).
 * A weight that is exactly 0 writes 0 for its term; that term gets no gradient and its work is skipped.
 * Gradient: to verts only.  With u_i = d_i / ||d_i|| (0 at d_i = 0):  d lap / d v_k = (1 / (B V)) (-u_k + sum over i in N(k) of u_i / deg(i))
 * (adjacency is symmetric).  For a quad, c = cos, g0 = -(n1^ - c n0^) / ||n0|| and likewise g1 are the gradients of 1 - cos with respect
 * to n0 and n1; for n = e x p the gradient with respect to p is g x e and with respect to e it is p x g; they are distributed onto
 * v0, v1, a, b with the sign of n1's definition.
 *
 * hifihr_mesh_topology_create builds the neighbour list (compressed rows), the quad table and the vertex -> (quad, role) list, checks
 * them and uploads them: the kernels take every index from these tables, no index is computed from a float.
 *   Refused (NULL returned, hifihr_last_error() says why): faces_host NULL, F <= 0, V <= 0, an index outside [0, V), a face that repeats a
 *   vertex, 4 Q >= 2^31.  A vertex that no face references is accepted (deg = 0).
 * hifihr_mesh_topology_destroy(NULL) is accepted.  hifihr_mesh_topology_counts writes V, E, Q (each pointer may be NULL); a NULL handle is
 *   refused.  hifihr_mesh_reg_partial_floats(NULL, .) and (h, B < 0) return 0; the size never decreases with B.
 * Compute entries -- refused (HIFIHR_EINVAL, nothing launched, nothing written): a NULL handle or pointer, B < 0, B V 3 >= 2^31, a weight
 *   that is not finite.  Accepted: B == 0 is a no-op (nothing launched, nothing written).
 * Precondition, NOT checked: finite vertices.  A NaN or an Inf gives unspecified values and gradients, never an out-of-range access.
 * Overwritten: hifihr_mesh_reg_fwd writes EVERY element of unit_d[B][V][3] (= u_i, which the backward reads; zeros when lam_lap == 0),
 *   of partial_d[hifihr_mesh_reg_partial_floats(h, B)] and of out_d[2].  hifihr_mesh_reg_bwd OVERWRITES every element of
 *   gverts_d[B][V][3]; it takes the gradients of the two terms as the DEVICE vector gout_d[2] and must be given the forward's weights.
 * Repeatable: no atomics.  Per-workgroup partial sums are folded by one workgroup in a fixed order, in double; in the backward every
 *   element has exactly one writer that sums in table order: out_d, unit_d and gverts_d have the same bits on every call.
 * No allocation and no synchronisation inside the compute entries: they can be captured into a hipGraph (creation allocates and copies:
 *   do it outside a capture). */
typedef struct hifihr_mesh_topology hifihr_mesh_topology_t;
hifihr_mesh_topology_t* hifihr_mesh_topology_create(const int32_t* faces_host, int F, int V);
int hifihr_mesh_topology_destroy(hifihr_mesh_topology_t* h);
int hifihr_mesh_topology_counts(const hifihr_mesh_topology_t* h, int* V, int* E, int* Q);
size_t hifihr_mesh_reg_partial_floats(const hifihr_mesh_topology_t* h, int B);
int hifihr_mesh_reg_fwd(const hifihr_mesh_topology_t* h, const float* verts_d, int B, float lam_lap, float lam_nc, float* unit_d,
                        float* partial_d, float* out_d, void* stream);
int hifihr_mesh_reg_bwd(const hifihr_mesh_topology_t* h, const float* verts_d, const float* unit_d, const float* gout_d, int B,
                        float lam_lap, float lam_nc, float* gverts_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Chamfer distance (csrc/chamfer.hip): the loss term `chamfer` and the evaluation metric of the same name.  It is the reference's
 * ChamferLoss (utils/losses_util.py:304-337, defined there and never wired: the import in losses.py:7 is commented out) with
 * mean(loss_1) + mean(loss_2) at unit weights, pinned by tests/golden/chamfer.npz, and PyTorch3D's chamfer_distance(x, y)[0] at its
 * defaults [recalled]: parity with PyTorch3D is unpinned.  tests/chamfer_ref.py restates the definition below in float64.
 *
 * Definition, per sample b, x = x_d[b] [N][3] (the prediction), y = y_d[b] [M][3] (the target), fp32 in, every operation in fp64:
 *   d2(i, j) = (dx dx + dy dy) + dz dz,   dx = (double)x[i][0] - (double)y[j][0], ...       this order, no contraction
 *   a[i] = the j that minimises (d2(i, j), j) lexicographically: ties go to the LOWEST index;   c[j] = the i that minimises (d2(i, j), i)
 *   sum_xy[b] = sum_i d2(i, a[i]),   sum_yx[b] = sum_j d2(c[j], j)
 *   value = w_xy mean_b (sum_xy[b] / N) + w_yx mean_b (sum_yx[b] / M), rounded to fp32 once
 * A direction whose weight is exactly 0 contributes exactly 0 and gets no gradient; its index and min arrays are still written.
 * Gradient (a and c are piecewise-constant choices), the inner sums in ascending index order, in fp64, rounded to fp32 once:
 *   gx[i] = gout ( w_xy 2 / (B N) (x[i] - y[a[i]]) + w_yx 2 / (B M) sum over { j : c[j] == i } of (x[i] - y[j]) )
 *   gy[j] = gout ( w_yx 2 / (B M) (y[j] - x[c[j]]) + w_xy 2 / (B N) sum over { i : a[i] == j } of (y[j] - x[i]) )
 * The library is built with -ffp-contract=off, so d2, a and c are the bits and integers of any float64 evaluation of the same expression.
 *
 * hifihr_chamfer_geometry writes the kernel's two constants (either pointer may be NULL): the queries one workgroup takes and the searched
 *   points of one LDS pass.  The four waves of a workgroup scan consecutive quarters of a pass.  For callers that size batches and for the
 *   tests, which build their cases round these boundaries.
 * hifihr_chamfer_workspace_bytes: the size of ws_d; 0 for B < 0 or N, M < 1; it never decreases with B.
 * Refused (HIFIHR_EINVAL, nothing launched, nothing written): a NULL among the required pointers (every pointer except gx_d, gy_d and
 *   stream), B < 0, N < 1, M < 1, a weight that is not finite, a grid beyond 2^31 - 1 workgroups (2 B ceil(max(N, M) / queries)).
 * Accepted: B == 0 is a no-op; hifihr_chamfer_bwd with gx_d == gy_d == NULL is a no-op; one of them NULL skips that set.
 * Overwritten: hifihr_chamfer_fwd writes EVERY element of idx_xy_d[B][N], idx_yx_d[B][M] (int32), min_xy_d[B][N], min_yx_d[B][M]
 *   (double: d2 at the arg-min), sums_d[B][2] (double: sum_xy, sum_yx) and out_d[1]; ws_d is scratch.  hifihr_chamfer_bwd OVERWRITES every
 *   element of gx_d[B][N][3] and gy_d[B][M][3]; a point that nobody chose gets its own term alone.  It takes the gradient of the value as the
 *   DEVICE scalar gout_d[1] and must be given the forward's weights and index arrays.
 * Repeatable: no atomics.  The search keeps (d2, index) pairs and compares them lexicographically wherever two candidates meet; partial
 *   sums are folded in a fixed order; the backward takes its scatter term as a gather with one writer per element: the same bits on every call.
 * Preconditions, NOT checked: finite coordinates.  A NaN or an Inf gives unspecified values, never an out-of-range access: an index starts
 *   at 0 and is only ever replaced by a loop counter, a d2 that is not a number never wins, and the backward clamps the indices it is given.
 * No allocation and no synchronisation inside the entries: they can be captured into a hipGraph. */
void hifihr_chamfer_geometry(int* queries_per_workgroup, int* tile_points);
size_t hifihr_chamfer_workspace_bytes(int B, int N, int M);
int hifihr_chamfer_fwd(const float* x_d, const float* y_d, int B, int N, int M, float w_xy, float w_yx, int32_t* idx_xy_d, int32_t* idx_yx_d,
                       double* min_xy_d, double* min_yx_d, double* sums_d, float* out_d, void* ws_d, void* stream);
int hifihr_chamfer_bwd(const float* x_d, const float* y_d, const int32_t* idx_xy_d, const int32_t* idx_yx_d, const float* gout_d, int B, int N,
                       int M, float w_xy, float w_yx, float* gx_d /* or NULL */, float* gy_d /* or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Point-to-mesh distance (csrc/point_mesh.hip): the loss term `point_mesh` and the evaluation metric of the same name, the squared distance
 * between a point cloud and the SURFACE of a triangle mesh.  At unit weights it is PyTorch3D's point_mesh_face_distance [recalled]: parity
 * with PyTorch3D is unpinned (no PyTorch3D is available here, and its min_triangle_area handling of small faces is not reproduced).
 * tests/point_mesh_ref.py restates the definition below in float64.
 *
 * Definition, per sample b: points p = p_d[b] [N][3], vertices v = v_d[b] [V][3], ONE face table faces_d [F][3] for the batch, whose
 * entries are clamped into [0, V) on load.  fp32 in, every operation in fp64, this order, no contraction; dot(x, y) = (x0 y0 + x1 y1) + x2 y2.
 *   the record of face f = (i0, i1, i2):  a = v[i0], ab = v[i1] - a, ac = v[i2] - a, abab = dot(ab, ab), abac = dot(ab, ac), acac = dot(ac, ac)
 *   for a point p:  ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = d1 - abab, d4 = d2 - abac, d5 = d1 - abac, d6 = d2 - acac
 *     vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, e1 = d1 - d3, e2 = d2 - d6, e3a = d4 - d3, e3b = d5 - d6, e3 = e3a + e3b,
 *     den = (va + vb) + vc
 *   the closest point cp(p, f) = a + (ab w1 + ac w2) of the triangle, by the region form of Ericson's closest-point-on-triangle (Real-Time
 *   Collision Detection, 5.1.5), the FIRST region whose test holds, weights (w0, w1, w2) of (i0, i1, i2):
 *     vertex a:  d1 <= 0 and d2 <= 0                                  (1, 0, 0)
 *     vertex b:  d3 >= 0 and d4 <= d3                                 (0, 1, 0)
 *     edge ab:   vc <= 0 and d1 >= 0 and d3 <= 0 and e1 > 0           (1 - q, q, 0),   q = d1 / e1
 *     vertex c:  d6 >= 0 and d5 <= d6                                 (0, 0, 1)
 *     edge ac:   vb <= 0 and d2 >= 0 and d6 <= 0 and e2 > 0           (1 - q, 0, q),   q = d2 / e2
 *     edge bc:   va <= 0 and e3a >= 0 and e3b >= 0 and e3 > 0         (0, 1 - q, q),   q = e3a / e3
 *     interior:  den > 0        q = 1 / den, w1 = clamp(vb q, 0, 1), w2 = clamp(vc q, 0, 1 - w1), w0 = (1 - w1) - w2
 *     otherwise (not reachable in exact arithmetic): vertex a
 *   Every denominator is guarded by its region's test, so there is no division by zero and no square root; every weight is >= 0 and they sum
 *   to 1 within an ulp.  A zero-area face (collinear or coincident vertices) has va = vb = vc = 0 in exact arithmetic and falls to the vertex
 *   and edge regions of the segment or point it degenerates to (an edge of length 0 is skipped by its guard): a finite distance, never a NaN.
 *   d2(p, f) = (dx dx + dy dy) + dz dz,   dx = ap0 - (ab0 w1 + ac0 w2), ...
 *   a[i] = the f that minimises (d2(p_i, f), f) lexicographically: ties go to the LOWEST index;  c[f] = the i that minimises (d2(p_i, f), i)
 *   sum_pf[b] = sum_i d2(p_i, a[i]),   sum_fp[b] = sum_f d2(p_c[f], f)
 *   value = w_pf mean_b (sum_pf[b] / N) + w_fp mean_b (sum_fp[b] / F), rounded to fp32 once
 * A direction whose weight is exactly 0 is NOT SEARCHED: it contributes exactly 0, gets no gradient, its index, weight and minimum arrays
 * are left untouched and its column of sums_d is written as 0.
 * Gradient: the choices a, c and the weights are constants (exact away from the region boundaries: the envelope property of the constrained
 * minimum).  With r(i, f) = p_i - cp computed as dx, dy, dz above from the STORED w1, w2, c_pf = w_pf 2 / (B N), c_fp = w_fp 2 / (B F), the
 * inner sums in ascending index order, in fp64, rounded to fp32 once:
 *   gp[i] = gout ( c_pf r(i, a[i]) + c_fp sum over { f : c[f] == i } of r(i, f) )
 *   slab[f][k] = -( c_pf sum over { i : a[i] == f } of w_k(i) r(i, f)  +  c_fp w_k(f) r(c[f], f) )           k = 0, 1, 2: the face's corners
 *   gv[u] = gout sum over the corners (f, k) with faces[f][k] == u, ascending in 3 f + k, of slab[f][k]
 * The library is built with -ffp-contract=off, so d2, a, c and the weights are the bits and integers of any float64 evaluation of the same
 * expressions (the one division per pair is IEEE-rounded).
 *
 * hifihr_point_mesh_geometry writes the kernels' four constants (any pointer may be NULL): the points one workgroup takes and the face
 *   records of one LDS pass (points -> faces), the faces one workgroup takes and the points of one LDS pass (faces -> points).  The four
 *   waves of a workgroup scan consecutive quarters of a pass.  The tests build their cases round these boundaries.
 * hifihr_point_mesh_workspace_bytes: the size of ws_d (partial sums, then the backward's per-corner slab of B F 9 doubles); 0 for B < 0 or
 *   N, V, F < 1; it never decreases with B.  Forward and backward take the same workspace size; the backward reads nothing the forward left.
 * v2c_off_d [V + 1], v2c_corner_d [3 F] (int32): the vertex -> corner table, built by the host once per face table: corner 3 f + k belongs
 *   to vertex faces[f][k]; v2c_corner lists the corners vertex by vertex, ascending inside a vertex; v2c_off[u] .. v2c_off[u + 1] is vertex
 *   u's range.  Entries are clamped on load.
 * Refused (HIFIHR_EINVAL, nothing launched, nothing written): a NULL among the required pointers (every pointer except gp_d, gv_d and
 *   stream), B < 0, N < 1, V < 1, F < 1, a weight that is not finite, a grid beyond 2^31 - 1 workgroups (B (ceil(N / points per
 *   workgroup) + ceil(F / faces per workgroup)), B ceil(max(N, V, F) / 256)).
 * Accepted: B == 0 is a no-op; hifihr_point_mesh_bwd with gp_d == gv_d == NULL is a no-op; one of them NULL skips that gradient.
 * Overwritten: hifihr_point_mesh_fwd writes, for every searched direction, EVERY element of idx_pf_d[B][N] / idx_fp_d[B][F] (int32),
 *   bary_pf_d[B][N][3] / bary_fp_d[B][F][3] (double: w0, w1, w2 at the arg-min), min_pf_d[B][N] / min_fp_d[B][F] (double: d2 at the
 *   arg-min); always sums_d[B][2] (double: sum_pf, sum_fp) and out_d[1]; ws_d is scratch.  hifihr_point_mesh_bwd OVERWRITES every element
 *   of gp_d[B][N][3] and gv_d[B][V][3] (a vertex of no face gets 0).  It takes the gradient of the value as the DEVICE scalar gout_d[1] and
 *   must be given the forward's weights, index and weight arrays.
 * Repeatable: no atomics.  The search keeps (d2, index) pairs and compares them lexicographically wherever two candidates meet; partial
 *   sums are folded in a fixed order; the backward takes both scatters as gathers with one writer per element: the same bits on every call.
 * Preconditions, NOT checked: finite coordinates.  A NaN or an Inf gives unspecified values, never an out-of-range access: an index starts
 *   at 0 and is only ever replaced by a loop counter, a d2 that is not a number never wins, and every index read from memory is clamped.
 * No allocation and no synchronisation inside the entries: they can be captured into a hipGraph. */
void hifihr_point_mesh_geometry(int* points_per_wg, int* faces_per_pass, int* faces_per_wg, int* points_per_pass);
size_t hifihr_point_mesh_workspace_bytes(int B, int N, int V, int F);
int hifihr_point_mesh_fwd(const float* p_d, const float* v_d, const int32_t* faces_d, int B, int N, int V, int F, float w_pf, float w_fp,
                          int32_t* idx_pf_d, double* bary_pf_d, double* min_pf_d, int32_t* idx_fp_d, double* bary_fp_d, double* min_fp_d,
                          double* sums_d, float* out_d, void* ws_d, void* stream);
int hifihr_point_mesh_bwd(const float* p_d, const float* v_d, const int32_t* faces_d, const int32_t* idx_pf_d, const double* bary_pf_d,
                          const int32_t* idx_fp_d, const double* bary_fp_d, const float* gout_d, const int32_t* v2c_off_d,
                          const int32_t* v2c_corner_d, int B, int N, int V, int F, float w_pf, float w_fp, float* gp_d /* or NULL */,
                          float* gv_d /* or NULL */, void* ws_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Texture-PCA decode (csrc/texpca.hip): tex[b][n] = mean[n] (or 0 when NULL) + sum_k coef[b][k] basis[k][n], K <= 32, n % 4 == 0.
 * The texture half of the NIMBLE layer as the reference consumes it (models_res_nimble.py:57,133-142: texture_params [B,10] -> the
 * hand's texture).  NIMBLE's own basis is not available: the caller supplies one (n = 778 * 3 vertex
 * colours for the declared stand-in, n = 1024 * 1024 * 3 for a UV map).  HBM-bound: 4 n (K + 1 + B) algorithmic bytes.
 * bwd: dcoef_zeroed_d[B][K] (ZERO on entry) += sum_n gtex[b][n] basis[k][n]   (float atomics: reproducible to rounding).
 * tex_d is OVERWRITTEN (no atomics: the same bits on every call); dcoef_zeroed_d is ACCUMULATED onto whatever it holds.
 * Refused (HIFIHR_EINVAL, nothing launched or written): B <= 0, K outside 1 .. 32, n < 4 or n % 4 != 0, a NULL pointer other than mean_d.
 * ---------------------------------------------------------------------------------------------- */
int hifihr_texture_pca_fwd(const float* coef_d, const float* basis_d, const float* mean_d /* or NULL */, int B, int K, long n,
                           float* tex_d, void* stream);
int hifihr_texture_pca_bwd(const float* gtex_d, const float* basis_d, int B, int K, long n, float* dcoef_zeroed_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient exchange of the data-parallel step (RCCL over xGMI), for callers that do not go through torch.distributed.
 * Replaces nn.DataParallel (reference train_hrnet.py:560): one process per GPU, the ONE collective
 * of a step is a SUM all-reduce of the flat fp32 gradient buffer (the 1 / world scale is hifihr_adam_step's grad_scale),
 * parameters are broadcast once at start.  librccl is resolved with dlopen at the first call (no link-time dependency).
 *   rank 0: hifihr_comm_get_unique_id(&uid), ship the 128 bytes to the other ranks out of band;
 *   every rank (its device current): hifihr_comm_init(&comm, rank, world, &uid); per step hifihr_comm_allreduce_f32(comm, grads_d,
 *   n, stream) -- any number of calls on slices of the buffer (buckets) -- then hifihr_adam_step; hifihr_comm_destroy at the end.
 * Errors: HIFIHR_EHIP with the RCCL message in hifihr_comm_last_error().
 * ---------------------------------------------------------------------------------------------- */
typedef struct hifihr_comm hifihr_comm;
typedef struct { char bytes[128]; } hifihr_comm_uid;
const char* hifihr_comm_last_error(void);
int hifihr_comm_get_unique_id(hifihr_comm_uid* out);
int hifihr_comm_init(hifihr_comm** out, int rank, int world, const hifihr_comm_uid* uid);
int hifihr_comm_allreduce_f32(hifihr_comm* comm, float* buf_d /* in place */, size_t n, void* stream);
int hifihr_comm_broadcast_f32(hifihr_comm* comm, float* buf_d, size_t n, int root, void* stream);
int hifihr_comm_destroy(hifihr_comm* comm);

/* ------------------------------------------------------------------------------------------------
 * Fused Adam over ONE flat parameter buffer.
 * Replaces optimizer.step() of torch.optim.Adam(betas=(0.9,0.999), eps=1e-8, weight_decay=0|0.01)
 * reference train_hrnet.py:111-113, 546-551.  All four buffers are device fp32[n], 16-byte aligned.
 * grads are multiplied by grad_scale before use (1/world_size after a sum all-reduce).  `step` counts from 1.
 * Deterministic (no atomics on the data): the same inputs give the same bits.  A zero gradient on zero moments leaves the parameters
 * bit-identical at weight_decay 0 (0 / (0 + eps) = 0).
 * Refused (HIFIHR_EINVAL, nothing launched or written), by all three entries: a NULL buffer (state_d / dyn_d included), a buffer
 * that is not 16-byte aligned (state_d: 8-byte), and for hifihr_adam_step `step` < 1.
 * n = 0 is accepted by all three and is NOT a step: nothing is launched, nothing is written, and hifihr_adam_step_counted's
 * counter and running products stay as they are.
 * ---------------------------------------------------------------------------------------------- */
int hifihr_adam_step(float* params_d, const float* grads_d, float* exp_avg_d, float* exp_avg_sq_d, size_t n,
                     float grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                     void* stream);
/* Same update with the two per-step scalars read from DEVICE memory, dyn_d[2] = { lr / (1 - beta1^t),
 * 1 / sqrt(1 - beta2^t) }: the launch can be captured in a hipGraph and replayed while the host refreshes dyn_d
 * (a 8-byte async copy) outside the graph before each replay. */
/* The same update with the step counter and the learning rate in DEVICE memory (round 5): state_d is hifihr_adam_state_bytes() = 48 bytes,
 *   f64 lr, f64 beta1, f64 beta2, f64 beta1^step, f64 beta2^step, i32 step (completed steps), i32 0
 * written once by the caller (and again whenever lr or the counter changes: a scheduler step, a restored checkpoint).  The launch computes
 * lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t), t = step + 1, in double precision on the device (from the running products) and advances
 * `step` and the products when its last workgroup finishes: a captured training step replays with nothing to refresh from the host in between (hifihr_adam_step_dyn needs a 2-float upload
 * in front of every replay).  One launch at a time per state. */
size_t hifihr_adam_state_bytes(void);
int hifihr_adam_step_counted(float* params_d, const float* grads_d, float* exp_avg_d, float* exp_avg_sq_d, size_t n, float grad_scale,
                             float eps, float weight_decay, void* state_d, void* stream);
int hifihr_adam_step_dyn(float* params_d, const float* grads_d, float* exp_avg_d, float* exp_avg_sq_d, size_t n,
                         float grad_scale, float beta1, float beta2, float eps, float weight_decay, const float* dyn_d,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient guard for the fused Adam step: global L2 norm clipping and a skip on a non-finite gradient, all on the device (nothing is
 * read back, both calls can be captured in a hipGraph).  Where torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) and a
 * skip-on-overflow step would sit in front of optimizer.step(), reference train_hrnet.py:111-113.
 *   hifihr_grad_norm(grads_d, n, grad_scale, max_norm, guard_d, ws_d): two launches -- per-workgroup sums of g_i^2 (squares and sums in
 *     double: a finite fp32 gradient never overflows them) into ws_d, then one workgroup that folds them and writes guard_d.  Every
 *     summation order is fixed: the same input gives the same bits.
 *   hifihr_adam_step_guarded(..., state_d, guard_d): the Adam update of hifihr_adam_step (state_d NULL: lr, beta*, step from the host) or
 *     of hifihr_adam_step_counted (state_d given: lr, beta1, beta2 and step are ignored), reading {coef, finite} from guard_d.
 * guard_d: hifihr_grad_guard_bytes() = 32 bytes, 8-byte aligned, zeroed ONCE by the caller:
 *   f64 norm      sqrt(sum (grad_scale g_i)^2) of the last norm pass (alignment padding inside grads_d must be zero)
 *   f32 coef      min(1, max_norm / (norm + 1e-6)) as clip_grad_norm_ forms it; exactly 1.0f for max_norm = +inf; 0 when not finite
 *   i32 finite    1 when the sum of squares is finite, 0 when any element is NaN or +-inf
 *   i32 steps, i32 clipped (coef < 1), i32 skipped (not finite): running counts, advanced by every norm pass
 *   i32 padding
 * ws_d: hifihr_grad_norm_workspace_bytes(n) bytes, 8-byte aligned, contents irrelevant.
 * finite:     the update runs with grad_scale * coef (one f32 product) in the place of grad_scale; weight decay is added after, as in
 *             the unguarded entries.  coef == 1.0f gives the bits of hifihr_adam_step / hifihr_adam_step_counted on the same inputs.
 * not finite: the step is SKIPPED -- params, exp_avg and exp_avg_sq keep their bits, no weight decay -- but it still COUNTS: the counted
 *             state's step and running products advance exactly as in hifihr_adam_step_counted, and a host-scalar caller keeps
 *             incrementing `step`.  (torch.cuda.amp.GradScaler does not count a skipped step; here the host never reads the flag back,
 *             so lr schedule, checkpoint step and data-parallel ranks stay aligned.  The price is a bias correction one step ahead.)
 * Data parallel: call hifihr_grad_norm after the all-reduce with the same grad_scale the Adam call gets; every rank sees the same bits.
 * Refused (HIFIHR_EINVAL, nothing launched or written): a NULL pointer (state_d excepted: it selects the form); grads_d (and for the
 * step the other three buffers) not 16-byte aligned; guard_d, ws_d or state_d not 8-byte aligned; max_norm NaN or <= 0 (+inf is
 * accepted: guard only); a non-finite grad_scale; step < 1 when state_d is NULL.
 * n = 0 is accepted by both and is NOT a step: nothing is launched, nothing written, no counter moves.
 * ---------------------------------------------------------------------------------------------- */
size_t hifihr_grad_guard_bytes(void);
size_t hifihr_grad_norm_workspace_bytes(size_t n);
int hifihr_grad_norm(const float* grads_d, size_t n, float grad_scale, float max_norm, void* guard_d, void* ws_d, void* stream);
int hifihr_adam_step_guarded(float* params_d, const float* grads_d, float* exp_avg_d, float* exp_avg_sq_d, size_t n, float grad_scale,
                             float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* state_d,
                             const void* guard_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * NHWC fp32 convolution on the f32 matrix cores (implicit GEMM, exact fp32 accumulate).
 * Replaces the cuDNN/MIOpen dispatches of the encoder's nn.Conv2d layers (forward, backward-data,
 * backward-weight): reference network/res_encoder.py:364-373 (ResNet trunk built at :345-362).
 * Layouts: x[N][H][W][C], w[K][R][S][C] (= a torch [K,C,R,S] tensor in channels_last memory format),
 * y[N][OH][OW][K] with OH = (H + 2 pad - R)/stride + 1.  C % 4 == 0; bwd_data needs K % 4 == 0 (K % 16 == 0 when stride > 1), bwd_weight K % 4 == 0.
 *
 * Workspace (ws_d / ws_bytes, may be NULL / 0): fwd, fwd_bnstats and bwd_data can run a BALANCED schedule -- exactly
 * 4 persistent workgroups per CU, each walking an equal share of the (tile, K-chunk) iterations, partial tiles summed
 * through ws_d -- instead of one workgroup per output tile, whose cost is quantised to whole rounds of 1024 workgroups
 * (784 tiles cost as much as 1024).  ws_d must hold hifihr_conv2d_workspace_bytes(...) bytes (0 = this shape never uses
 * one), be ALL ZERO before its first use and is returned all zero (self-cleaning); calls sharing a workspace must be
 * ordered on one stream.  Without a workspace the calls fall back to the data-parallel grid (same results up to fp32
 * summation order across K segments).
 * ---------------------------------------------------------------------------------------------- */
size_t hifihr_conv2d_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int bwd_data);
/* act: 0 = none, 1 = ReLU after the bias (nn.Conv2d + nn.ReLU of the LightEstimator, network/res_encoder.py:150-210; its
 * backward first runs hifihr_bias_relu_bwd: g = dy * (y > 0) (g_d may alias dy_d), db_acc_d[K] += column sums of g). */
int hifihr_conv2d_fwd(const float* x_d, const float* w_d, const float* bias_d /* [K] or NULL */, int act, float* y_d, int N,
                      int H, int W, int C, int K, int R, int S, int stride, int pad, void* ws_d, size_t ws_bytes, void* stream);
int hifihr_bias_relu_bwd(const float* dy_d, const float* y_d, long M, int C, float* g_d, float* db_acc_d /* or NULL */,
                         void* stream);
/* LightEstimator.forward's last two lines (reference network/res_encoder.py:205-210): lights[B][6] ->
 * colors[B][3] = hardtanh(lights[:, :3]) (nn.Hardtanh: clamp to [-1, 1]), directions[B][3] = lights[:, 3:], contiguous, one launch;
 * bwd: glights[B][6] = [gcolors where -1 < lights < 1 else 0, gdirections] (either gradient may be NULL = zero). */
int hifihr_light_split_fwd(const float* lights_d, int B, float* colors_d, float* directions_d, void* stream);
int hifihr_light_split_bwd(const float* lights_d, const float* gcolors_d, const float* gdirections_d, int B, float* glights_d,
                           void* stream);
/* dx[N][H][W][C] (overwritten).  wt_scratch_d: K*R*S*C floats of scratch (receives the [C][R][S][K] transpose).
 * A STRIDED filter of more than 62 taps onto an NHWC4 image (R * S > 62, stride > 1, C == 4, K % 16 == 0, ceil(R / stride) ceil(S / stride) K
 * <= 1024: the 11x11 / stride 4 AlexNet stem of the `lpips` loss term) runs on a direct gather from w_d itself (csrc/lpips.hip; fixed summation order, no workspace, wt_scratch_d untouched) -- the implicit-GEMM gather
 * holds 62 taps; the pre-transposed entries (_pre, _pre_res, _pre_plus1x1) do not serve such a filter. */
int hifihr_conv2d_bwd_data(const float* dy_d, const float* w_d, float* dx_d, float* wt_scratch_d, int N, int H, int W, int C,
                           int K, int R, int S, int stride, int pad, void* ws_d, size_t ws_bytes, void* stream);
/* dw[K][R][S][C] += sum over pixels (ACCUMULATES with fp32 atomics: zero it, or pass the gradient buffer). */
int hifihr_conv2d_bwd_weight(const float* x_d, const float* dy_d, float* dw_d, int N, int H, int W, int C, int K, int R, int S,
                             int stride, int pad, void* stream);
/* The same with caller-provided scratch: layer 1's 3x3 and the stem's 7x7 weight gradients are summed from per-workgroup slabs in a
 * fixed order (bit-reproducible, no atomics; csrc/conv_halo.hip).  ws: hifihr_conv2d_wgrad_workspace_bytes(...) bytes, any contents,
 * not shared with a launch that may run concurrently on another stream; 0 bytes needed = the shape runs on the atomics kernel.
 * Without it (hifihr_conv2d_bwd_weight) those shapes use scratch the library allocates on first use outside a stream capture. */
size_t hifihr_conv2d_wgrad_workspace_bytes(int N, int H, int W, int C, int K, int R, int S, int stride, int pad);
int hifihr_conv2d_bwd_weight_ws(const float* x_d, const float* dy_d, float* dw_accumulate_d, int N, int H, int W, int C, int K, int R, int S,
                                int stride, int pad, void* ws_d, size_t ws_bytes, void* stream);
/* The stem as the reference declares it, nn.Conv2d(3, 64, 7, 2, 3) (vendored resnet.py conv1): the image arrives as NHWC4 with a
 * zero fourth plane (hifihr_image_to_nhwc4), the parameter and its gradient keep 3 channels, dw3_d[K][R][S][3] (accumulated into).
 * Served by the slab kernel only (7x7, stride 2, pad 3, K = 64; ask _supported); ws as hifihr_conv2d_wgrad_workspace_bytes(.., C = 4, ..).
 * The forward's padded filter [K][R][S][4] comes out of hifihr_weight_prep (job kind 5). */
int hifihr_conv2d_bwd_weight_c3_supported(int N, int H, int W, int K, int R, int S, int stride, int pad);
int hifihr_conv2d_bwd_weight_c3(const float* x4_d, const float* dy_d, float* dw3_d, int N, int H, int W, int K, int R, int S, int stride,
                                int pad, void* ws_d, size_t ws_bytes, void* stream);
/* Winograd F(m x m, 3x3) for stride-1, pad-1 3x3 convolutions with many channels; m is the output-tile edge, 2 (csrc/wino.hip) or 4
 * (csrc/wino4.hip), P = (m + 2)^2 the positions of a tile (16 / 36) and T = hifihr_wino_tiles(N, H, W, m) the tiles.  2.25x (m = 2) / 4x
 * (m = 4) fewer multiplications than the direct kernel, results within 1e-5 of it (ResNet-18 layers 2-4, VGG19).  Forward:
 *   hifihr_wino_weight_transform(w[K][3][3][C], U[P][K][C], K, C, flip = 0, m)
 *   hifihr_wino_input_transform (x[N][H][W][C], V[P][T][C], ..., m)
 *   hifihr_wino_gemm            (V, U, M[P][T][K], ..., m)  -- P GEMMs on the matrix cores; ws of hifihr_wino_gemm_workspace_bytes or NULL
 *   hifihr_wino_output_transform(M, y[N][H][W][K], stats_d or NULL, ..., m)   -- stats_d: batch-norm slot buffer (zero on entry)
 * Backward-data is the same sequence on dy with the weights of the transposed, 180-degree rotated filter:
 *   weight_transform(wt[C][3][3][K] (= the [C][R][S][K] transpose hifihr_conv2d_bwd_data also builds), U'[P][C][K], C, K, flip = 1, m).
 * Backward-weight, from Y'[P][T][K] = hifihr_wino_dy_transform(dy) and V[P][T][C] (the forward's input transform of x): with
 *   parts = hifihr_wino_wgrad_parts(N, H, W, C, K, m) > 0 (the product is csrc/gemm.hip's: C % 64 == 0, K % 64 == 0)
 *     hifihr_wino_wgrad_gemm_parts(V, Y', du_parts[parts][P][K][C], ..., parts, m)  then
 *     hifihr_wino_dw_transform_parts: dw[K][3][3][C] += G^T (sum of the slabs) G   -- nothing zero-initialised, bit-reproducible;
 *   with parts == 0, at m = 2 only: hifihr_wino_wgrad_gemm: dU[16][K][C] (ZERO on entry) += the 16 reductions over the tiles (atomics), then
 *     hifihr_wino_dw_transform: dw[K][3][3][C] += G^T dU G  (accumulates, like hifihr_conv2d_bwd_weight).
 * All calls of one layer must use the same m, and every buffer is sized with its P and T.  ANY m other than 2 or 4 is refused with
 * HIFIHR_EINVAL by every entry that takes m, and the queries -- hifihr_wino_tiles, _tiles_computed, _gemm_workspace_bytes, _wgrad_parts --
 * answer 0 for it: no entry falls back to F(2x2, 3x3) on an m it does not know.
 * The transforms of both tile edges take ANY N, H, W > 0 -- images smaller than one tile included (H or W of 1, 2, 3 at m = 4: the tile is
 * zero-padded like any ragged last tile) -- and any C resp. K that is a multiple of 4; the weight and dw transforms any K > 0.  They write every
 * row t < hifihr_wino_tiles_computed of V / Y' and ZEROS into the rows behind it (the padding of the mosaic form); the output transforms read
 * rows t < hifihr_wino_tiles_computed of M only, and the products may leave the rows of M behind it unwritten.  act of the _act form is 0 or 1.
 * hifihr_wino_gemm: at m = 4 the product is csrc/gemm.hip's or refused (C % 32 == 0, K % 64 == 0); at m = 2 it needs C % 32 == 0 and
 * K % 4 == 0 and runs on csrc/gemm.hip where that takes the shape (K % 64 == 0), else on the gather kernel of csrc/conv.hip (ws then as for
 * hifihr_conv2d_fwd).  The products on csrc/gemm.hip (hifihr_wino_gemm, hifihr_wino4_bwd_gemm_pair) refuse, like hifihr_bgemm_nt, operands of
 * 2^31 elements or more per position (T * C, T * K, K * C) with HIFIHR_EINVAL.
 * (tests/test_hostsim_gemm_contract.py holds every entry to this, around a float64 product, against float64 conv2d.)
 * hifihr_wino_tile(N, H, W, C, K) returns the m this library prefers for a layer: 4 where the batched GEMMs of csrc/gemm.hip take the
 * shape in all three directions (C % 64 == 0, K % 64 == 0, H, W >= 4), else 2.  m = 4 has the slab form of backward-weight only
 * (hifihr_wino_wgrad_parts > 0).  The per-step weight re-layout (hifihr_weight_prep) has job kinds 1 / 2 for U[16][K][C] / U'[16][C][K] and
 * 3 / 4 for U[36][K][C] / U'[36][C][K]. */
int hifihr_wino_tile(int N, int H, int W, int C, int K);
/* T, the tiles (rows per position of V / M / Y') a layer has at tile edge m: N * ceil(H / m) * ceil(W / m) -- or, at m = 4 on square maps
 * with H % 4 in {1, 2} and N % 16 == 0, the tiles of the 4 x 4-image MOSAICS the transforms cut (16 images share one map with single
 * lines of zeros between them: 225 tiles per 16 images of 14 x 14 instead of 256), rounded up to a multiple of 32.  Every buffer of the
 * pipeline is sized with it.  (HIFIHR_WINO_MOSAIC=0: always the first form.) */
long hifihr_wino_tiles(int N, int H, int W, int m);
/* ... and the rows of them the forward / backward-data products actually compute (the mosaic count before the rounding; else the same). */
long hifihr_wino_tiles_computed(int N, int H, int W, int m);
size_t hifihr_wino_gemm_workspace_bytes(int N, int H, int W, int C, int K, int m);
int hifihr_wino_wgrad_parts(int N, int H, int W, int C, int K, int m);
int hifihr_wino_weight_transform(const float* w_d, float* u_d, int K, int C, int flip, int m, void* stream);
int hifihr_wino_input_transform(const float* x_d, float* v_d, int N, int H, int W, int C, int m, void* stream);
int hifihr_wino_dy_transform(const float* dy_d, float* yt_d, int N, int H, int W, int K, int m, void* stream);
/* Backward of a Winograd layer reads dy twice (input transform for backward-data, hifihr_wino_dy_transform for backward-weight);
 * this does both from one read: v_d[P][T][K] = B^T d B of the padded (m + 2)^2 patches, yt_d[P][T][K] = A dy A^T of their central m x m. */
int hifihr_wino_input_dy_transform(const float* dy_d, float* v_d, float* yt_d, int N, int H, int W, int K, int m, void* stream);
int hifihr_wino_gemm(const float* v_d, const float* u_d, float* m_d, int N, int H, int W, int C, int K, int m, void* ws_d, size_t ws_bytes,
                     void* stream);
int hifihr_wino_output_transform(const float* m_d, float* y_d, float* stats_d /* or NULL */, int N, int H, int W, int K, int m, void* stream);
/* Output transform with the act epilogue of hifihr_conv2d_fwd: y = act(A^T m A + bias[K] (or NULL)), act 0 = none, 1 = ReLU
 * (VGG19 layers of the perceptual loss, reference utils/perceptual_loss.py:27-36). */
int hifihr_wino_output_transform_act(const float* m_d, float* y_d, const float* bias_d /* or NULL */, int act, int N, int H, int W, int K,
                                     int m, void* stream);
/* Output transform of a BACKWARD-DATA product whose layer input was a ReLU's output (VGG19 conv + ReLU -> conv): y_d = mask_d > 0 ? A^T m A : 0
 * with mask_d[N][H][W][K] = that ReLU output (the layer's saved input) -- the ReLU's backward where its gradient is produced, instead of a
 * hifihr_bias_relu_bwd pass in front of the previous layer's backward.  m == 4 only. */
int hifihr_wino_output_transform_mask(const float* m_d, float* y_d, const float* mask_d, int N, int H, int W, int K, int m, void* stream);
int hifihr_wino_wgrad_gemm_parts(const float* v_d, const float* yt_d, float* du_parts_d, int N, int H, int W, int C, int K, int parts, int m,
                                 void* stream);
int hifihr_wino_dw_transform_parts(const float* du_parts_d, int parts, float* dw_acc_d, int K, int C, int m, void* stream);
int hifihr_wino_wgrad_gemm(const float* v_d, const float* yt_d, float* du_zeroed_d, int N, int H, int W, int C, int K, void* stream);
int hifihr_wino_dw_transform(float* du_d, float* dw_acc_d, int K, int C, int clear_du /* 1: leave du_d all zero (self-cleaning) */,
                             void* stream);
/* 3x3 / stride 1 / pad 1 convolution with 64 input and 64 output channels as Winograd F(2x2, 3x3) in ONE launch, the transforms in
 * registers and nothing of the transform domain in HBM (round 3, csrc/conv_halo.hip: conv_wino2_kernel) -- ResNet layer 1 (reference
 * network/res_encoder.py:364-373 -> torchvision BasicBlock conv1 / conv2 of layer1) and VGG19 conv1_2 of the perceptual loss (reference
 * utils/perceptual_loss.py:27-36).  u_d = U[16][64][64]: hifihr_wino_weight_transform(w, u, 64, 64, 0, 2) or hifihr_weight_prep kind 1 for
 * the forward; kind 2 (the transposed, rotated filter) with x_d = dy gives backward-data.  bias_d / relu: epilogue (VGG19); stats_d: the
 * forward statistics slots of the batch norm that follows (hifihr_bn_stats_floats(64) floats, zeroed) or NULL.  H even, W even and >= 14
 * (hifihr_conv3x3_c64_wino_supported); results within 1e-5 (relative to the output scale) of the direct convolution. */
int hifihr_conv3x3_c64_wino_supported(int N, int H, int W, int C, int K);
/* 1 when the library's page of zeros for this device exists (or could be allocated now: `stream` is not capturing).  The kernels whose
 * loaders read out-of-image taps from it (hifihr_conv3x3_c64_wino, the ragged / gathering row-share GEMM) cannot allocate it inside a stream
 * capture: a caller that is about to capture asks here first and otherwise picks the kernels that do not need it. */
int hifihr_zero_page_ready(void* stream);
int hifihr_conv3x3_c64_wino(const float* x_d, const float* u_d, const float* bias_d /* or NULL */, int relu, float* y_d,
                            float* stats_d /* or NULL */, int N, int H, int W, void* stream);
/* The same launch with y = product + res_d[N][H][W][64] (round 4).  Backward-data of a layer whose input has a SECOND consumer -- the
 * identity branch of a residual block (reference torchvision BasicBlock: `out += identity`, network/res_encoder.py:364-373): autograd adds
 * the two gradients of that input in an elementwise pass of its own; here the other consumer's gradient is added where this one is produced. */
int hifihr_conv3x3_c64_wino_res(const float* x_d, const float* u_d, const float* res_d, float* y_d, int N, int H, int W, void* stream);
/* Both gradients of one such layer in ONE launch (round 5): dx_d = hifihr_conv3x3_c64_wino[_res](dy_d, u_bwd_d [, res_d or NULL]) -- u_bwd_d the
 * Winograd-domain filters of the transposed convolution (hifihr_weight_prep kind 2) -- and dw_d[64][3][3][64] += the weight gradient of
 * hifihr_conv2d_bwd_weight(x_d, dy_d) (the pixel-reduction slab kernel + its fixed-order slab sum).  The two halves are independent,
 * ~50 and ~65 us at the config batch: separately each pays its own ramp-up and tail, here the workgroups of one launch are split between
 * them.  Results are those of the separate calls up to the summation order over workgroup shares (the weight gradient stays
 * bit-reproducible run to run).  ws_d: scratch of hifihr_conv2d_bwd_weight_ws_bytes or NULL (library-owned).  Replaces, for ResNet layer 1
 * (reference utils/Freihand_GNN_mano/network/resnet.py BasicBlock convs at 56 x 56 x 64), the pair of autograd nodes
 * cudnn_convolution_backward_input / _weight. */
int hifihr_conv3x3_c64_bwd_pair_supported(int N, int H, int W);
int hifihr_conv3x3_c64_bwd_pair(const float* dy_d, const float* u_bwd_d, const float* res_d /* or NULL */, float* dx_d, const float* x_d,
                                float* dw_d, void* ws_d, size_t ws_bytes, int N, int H, int W, void* stream);
/* The same pair launch with the slab sum LEFT to the caller: the weight-gradient slabs stay in slabs_d ([*nslab][9][64][64], slab_bytes >=
 * hifihr_conv2d_wgrad_workspace_bytes of the layer) and hifihr_conv_halo_wgrad_reduce_multi adds the slabs of several layers to their
 * dw_acc_d[64][3][3][64] in ONE launch, slabs in slab order (bit-identical to the sum hifihr_conv3x3_c64_bwd_pair makes itself).  A step
 * whose weight gradients are read by the optimizer only defers the sums of its 64 -> 64 layers to one call in front of it. */
int hifihr_conv3x3_c64_bwd_pair_slabs(const float* dy_d, const float* u_bwd_d, const float* res_d /* or NULL */, float* dx_d, const float* x_d,
                                      void* slabs_d, size_t slab_bytes, int N, int H, int W, int* nslab /* host, out */, void* stream);
typedef struct hifihr_halo_reduce_job {
  const float* slabs_d;
  float* dw_acc_d;
  int nslab;
} hifihr_halo_reduce_job;
int hifihr_conv_halo_wgrad_reduce_multi(const hifihr_halo_reduce_job* jobs /* host array */, int njobs, void* stream);
/* Batch-norm fused into the F(4x4, 3x3) input transform (round 3, csrc/wino4_bn.hip).  For a BatchNorm2d whose consumer is a Winograd
 * convolution (reference BasicBlock: conv1 -> bn1 -> relu -> conv2; bn2 -> += identity -> relu -> the next block's conv1,
 * network/res_encoder.py:364-373 + vendored utils/Freihand_GNN_mano/network/resnet.py) this ONE launch replaces hifihr_bn_act_fwd followed by
 * hifihr_wino_input_transform: x_d is the RAW output of the previous convolution, stats_d its batch statistics (consumed: zero on
 * return, as in hifihr_bn_act_fwd, same save_mean / save_invstd / running-statistics semantics); the activation a = relu(bn(x) + residual?)
 * is formed on the fly and only V = B^T a B is written.  With residual_d, out_d (same shape as x) receives a as well -- the next block's
 * identity branch reads it; without, both are NULL and a is never stored (the backward recomputes the ReLU mask from x, as
 * hifihr_bn_act_bwd does with y_d = NULL).  m = 4 and C % 4 == 0, C <= 512 (hifihr_wino_bn_input_supported). */
int hifihr_wino_bn_input_supported(int C, int m);
int hifihr_wino_bn_input_transform(const float* x_d, float* stats_d, const float* gamma_d, const float* beta_d, const float* residual_d,
                                   float* out_d, float* v_d, int N, int H, int W, int C, int m, float eps, float momentum,
                                   float* save_mean_d, float* save_invstd_d, float* running_mean_d, float* running_var_d, void* stream);
/* The backward of that fusion (round 3): the batch-norm backward no longer makes passes of its own over the gradient.
 *   hifihr_wino_output_transform_bnred: output transform of the backward-data product m_d[36][T][C] of the consuming convolution
 *     = d loss / d a; in its epilogue + gadd_d (the gradient that reached the block output through the next block's identity
 *     branch, or NULL), the ReLU mask (out_d > 0 when the forward added a residual, else recomputed from x_d), g_d = the masked
 *     gradient written once, and the batch-norm backward REDUCTION (sum g, sum g xhat) added into red_d (hifihr_bn_stats_floats(C)
 *     floats, all zero on entry).  Replaces hifihr_wino_output_transform + the autograd add + the reduction half of hifihr_bn_act_bwd.
 *   then EITHER hifihr_bn_bwd_apply: the apply half of hifihr_bn_act_bwd on (g_d, red_d): dx, dgamma_acc += , dbeta_acc +=, red_d zeroed;
 *   OR, when the batch-norm's input was itself produced by a Winograd convolution, hifihr_wino_bn_bwd_dual_transform in THAT
 *     convolution's backward: dy = gamma invstd (g - mean g - xhat mean(g xhat)) is evaluated on the fly and only V' = B^T dy B and
 *     Y' = A dy A^T are written (y_d = the convolution's raw output = the batch-norm's input; same dgamma / dbeta / red_d semantics).
 * Mirrors, in one direction each, torch.autograd through nn.BatchNorm2d + ReLU + `+= identity` of the reference's BasicBlock
 * (vendored utils/Freihand_GNN_mano/network/resnet.py).  m = 4, channels % 4 == 0 and <= 512. */
int hifihr_wino_output_transform_bnred(const float* m_d, const float* x_d, const float* out_d /* or NULL */, const float* gadd_d /* or NULL */,
                                       const float* save_mean_d, const float* save_invstd_d, const float* gamma_d, const float* beta_d,
                                       float* red_d, float* g_d, int N, int H, int W, int C, int m, void* stream);
int hifihr_wino_bn_bwd_dual_transform(const float* g_d, const float* y_d, const float* save_mean_d, const float* save_invstd_d,
                                      const float* gamma_d, float* red_d, float* v_d, float* yt_d, int N, int H, int W, int K, int m,
                                      float* dgamma_acc_d, float* dbeta_acc_d, void* stream);
int hifihr_bn_bwd_apply(const float* g_d, const float* x_d, const float* save_mean_d, const float* save_invstd_d, const float* gamma_d, long M,
                        int C, float* red_d, float* dx_d, float* dgamma_acc_d, float* dbeta_acc_d, void* stream);
/* The two products of a Winograd F(4x4, 3x3) layer's backward that do not depend on each other, in ONE launch (round 5):
 *   backward-data   M2[36][T][C] = V2[36][T][K] . U2[36][C][K]^T      (= hifihr_wino_gemm(V2, U2, M2, N, H, W, K, C, 4, ...))
 *   backward-weight dU_parts     = Yt[36][T][K]^T . Vx[36][T][C]      (= hifihr_wino_wgrad_gemm_parts(Vx, Yt, dU_parts, ..., parts, 4))
 * with V2 / Yt the two transforms of dy and Vx the forward's transformed input (the layer maps C -> K channels).  Workgroups of one
 * launch split between the two (a short launch of these kernels is shaped by its start and its end); falls back to the two launches
 * for shapes that are not on the row-share kernels.  Results identical to the separate calls. */
int hifihr_wino4_bwd_gemm_pair_supported(int N, int H, int W, int C, int K);   /* 1: the call below pairs; 0: it makes the two launches */
int hifihr_wino4_bwd_gemm_pair(const float* V2_d, const float* U2_d, float* M2_d, const float* Vx_d, const float* Yt_d, float* dU_parts_d,
                               int N, int H, int W, int C, int K, int parts, void* stream);
/* The same F(4x4, 3x3) weight-gradient transform (m = 4) for SEVERAL layers in one launch: dw_acc_d[K][3][3][C] += G^T (sum of the `parts`
 * slabs du_parts_d[parts][36][K][C]) G per job, jobs independent of each other.  `jobs` is a HOST array (its pointers are device pointers);
 * the entries travel in the kernel arguments, so nothing is uploaded and a captured launch keeps them.  Results identical to one
 * hifihr_wino_dw_transform_parts(..., 4, ...) call per job.  A training step whose weight gradients are only read by the optimizer
 * collects its layers' jobs during backward and makes this one call in front of the optimizer (reference train_hrnet.py:104-105). */
typedef struct hifihr_wino_dw_job {
  const float* du_parts_d;
  float* dw_acc_d;
  int parts, K, C;
} hifihr_wino_dw_job;
int hifihr_wino4_dw_transform_multi(const hifihr_wino_dw_job* jobs, int njobs, void* stream);
/* Batched fp32 GEMM on the f32 matrix cores (csrc/gemm.hip): the plain products a Winograd layer consists of -- the GEMM half of
 * the vendor-library call behind one conv2d of the reference (network/res_encoder.py:364-373).  hifihr_wino_gemm dispatches here
 * when the shape allows (C % 32 == 0, K % 64 == 0).
 *   hifihr_bgemm_nt: c[b][M][N] = a[b][M][K] . b[b][N][K]^T          (K % 32 == 0, N % 64 == 0, any M); with a workspace of
 *                    hifihr_bgemm_nt_workspace_bytes (zero-initialised once, handed back all zero) large shapes run on the persistent,
 *                    balanced kernel (one workgroup per CU, stream-K shares), else one workgroup per tile
 *   hifihr_bgemm_tn: c_parts[z][b][M][N] = sum over the t rows of slab z of a[b][t][M] (x) b[b][t][N]   (M, N % 64 == 0, any T);
 *                    `parts` = hifihr_bgemm_tn_parts(M, N, T, batch) slabs, to be summed by the consumer (no atomics).
 *                    Slab z holds the rows  32 cps z <= t < min(T, 32 cps (z + 1)),  cps = ceil(ceil(T / 32) / parts)  chunks of 32 rows
 *                    per slab; no slab is empty, every element of every slab is written (overwritten, not accumulated).
 * The contract of these entries (tests/test_hostsim_gemm_contract.py):
 *   - M, N, K / T, batch > 0 and the multiples above, non-null a, b, c; hifihr_bgemm_nt also M * K < 2^31 and N * K < 2^31 (the kernels
 *     index one problem's operand with 32-bit element offsets).  Anything else: HIFIHR_EINVAL, nothing written.
 *   - hifihr_bgemm_tn takes exactly parts == hifihr_bgemm_tn_parts(M, N, T, batch); any other count (0, parts + 1, ...) is HIFIHR_EINVAL.
 *     hifihr_bgemm_tn_parts answers 0 for a shape hifihr_bgemm_tn refuses.
 *   - hifihr_bgemm_nt_workspace_bytes answers 0 for a shape that needs no workspace or that hifihr_bgemm_nt refuses.  A workspace that is
 *     NULL or smaller than that is not an error: the product runs with one workgroup per tile and the workspace is not touched.
 *   - hifihr_bgemm_nt writes every element of c once and reads nothing of it; operands are read inside a[b][M][K] / b[b][N][K] only.
 *   - hifihr_bgemm_describe: out non-null, cap >= 8, batch > 0, else HIFIHR_EINVAL; "" for a shape the product entries refuse.
 *   - two calls on the same operands give the same bits (no atomics; the stream-K kernel hands its tiles over in a fixed order). */
size_t hifihr_bgemm_nt_workspace_bytes(int M, int N, int K, int batch);
int hifihr_bgemm_nt(const float* a_d, const float* b_d, float* c_d, int M, int N, int K, int batch,
                    void* ws_d /* zero-initialised, self-cleaning; or NULL */, size_t ws_bytes, void* stream);
int hifihr_bgemm_tn_parts(int M, int N, int T, int batch);
/* The schedule hifihr_bgemm_tn walks this shape on, measurement only (like hifihr_bgemm_describe: the kernel's name and the results are the
 * same either way): r > 0 -- the XCD-coherent one, an XCD owning r problems per round; 0 -- contiguous shares (a shape or a workgroup
 * count the schedule does not fit, a kernel other than the row-share one, HIFIHR_GEMM_TN_COHERENT=0) or a shape hifihr_bgemm_tn refuses. */
int hifihr_bgemm_tn_coherent(int M, int N, int T, int batch);
/* Name of the kernel instantiation a shape runs on, as a profiler lists it ("" when the shape is not supported): measurement only. */
int hifihr_bgemm_describe(int tn, int M, int N, int K_or_T, int batch, char* out, int cap);
int hifihr_bgemm_tn(const float* a_d, const float* b_d, float* c_parts_d, int M, int N, int T, int batch, int parts, void* stream);
/* [K][RS][C] -> [C][RS][K] (the transpose backward-data consumes).  K, RS, C > 0 (any values: no multiple is required), non-null pointers,
 * else HIFIHR_EINVAL; every element of wt_d is written once. */
int hifihr_weight_transpose(const float* w_d, float* wt_d, int K, int RS, int C, void* stream);
/* hifihr_conv2d_bwd_data on weights that are ALREADY transposed to [C][R][S][K] (hifihr_weight_transpose / hifihr_weight_prep). */
int hifihr_conv2d_bwd_data_pre(const float* dy_d, const float* wt_d, float* dx_d, int N, int H, int W, int C, int K, int R, int S,
                               int stride, int pad, void* ws_d, size_t ws_bytes, void* stream);
/* dx = backward-data + res_d[N][H][W][C] (round 4; see hifihr_conv3x3_c64_wino_res): the first block of a ResNet stage sends its input to
 * the strided 3x3 convolution AND the 1x1 downsample convolution -- the second backward-data adds the first one's result as it stores. */
int hifihr_conv2d_bwd_data_pre_res(const float* dy_d, const float* wt_d, const float* res_d, float* dx_d, int N, int H, int W, int C, int K,
                                   int R, int S, int stride, int pad, void* ws_d, size_t ws_bytes, void* stream);
/* dx = backward-data of the strided convolution (dy_d, wt_d as in hifihr_conv2d_bwd_data_pre) + backward-data of a SECOND convolution of the same
 * input: 1x1, the same stride, pad 0, the same channel counts (dy2_d [N][OH][OW][K], wt2_d [C][K] = its transposed filter) -- the downsample
 * branch of a residual stage's first block (reference: vendored torchvision BasicBlock, network/res_encoder.py:364-373 runs both through
 * cuDNN / MIOpen and autograd adds the two gradients).  The 1x1 convolution's gradient lands on the pixels (stride i, stride j) only: it is one
 * more tap of that parity class of the strided launch instead of a launch of its own plus a residual pass (round 6).
 * _supported: 1 when the shape runs on that path (stride >= 2, K % 16 == 0, C % 4 == 0, equal output grids, pad < R and pad < S -- so that
 * parity class (0, 0) has both tap rows and tap columns); HIFIHR_DGRAD_PLUS1X1=0 switches it off.  The call refuses every other shape. */
int hifihr_conv2d_bwd_data_pre_plus1x1_supported(int N, int H, int W, int C, int K, int R, int S, int stride, int pad);
int hifihr_conv2d_bwd_data_pre_plus1x1(const float* dy_d, const float* wt_d, const float* dy2_d, const float* wt2_d, float* dx_d, int N, int H,
                                       int W, int C, int K, int R, int S, int stride, int pad, void* stream);
/* dw_d[K][R][S][C] += weight gradient of the strided convolution, dw2_d[K][C] += weight gradient of the 1x1 / same stride / pad 0 convolution of
 * the same input with the same output channels (dy2_d [N][OH][OW][K]), in ONE launch: the second convolution's patch column is tap (pad, pad)
 * of the first (round 6; the downsample branch of a residual stage's first block, as hifihr_conv2d_bwd_data_pre_plus1x1).  Float atomics, like
 * hifihr_conv2d_bwd_weight on these shapes.  _supported: 1 when the shape runs on that path; HIFIHR_WGRAD_PLUS1X1=0 switches it off. */
int hifihr_conv2d_bwd_weight_plus1x1_supported(int N, int H, int W, int C, int K, int R, int S, int stride, int pad);
int hifihr_conv2d_bwd_weight_plus1x1(const float* x_d, const float* dy_d, float* dw_d, const float* dy2_d, float* dw2_d, int N, int H, int W,
                                     int C, int K, int R, int S, int stride, int pad, void* stream);
/* Every per-step weight re-layout of a model in ONE launch.  The weights change once per optimizer step; a ResNet-18 step
 * otherwise spends ~40 tiny launches (~5 us of launch floor each) on transposes and Winograd weight transforms.
 * jobs_d: DEVICE array of njobs descriptors (src / dst are device pointers);
 *   kind 0: dst[C][RS][K] = transpose of src[K][RS][C]                                   (= hifihr_weight_transpose)
 *   kind 1: dst = U[16][K][C] of src[K][3][3][C]                                         (= hifihr_wino_weight_transform, flip 0)
 *   kind 2: dst = U'[16][C][K], the backward-data weights of src[K][3][3][C]              (= weight_transpose + transform, flip 1)
 *   kind 3 / 4: the F(4x4, 3x3) forms of 1 / 2, U[36][K][C] / U'[36][C][K]
 *   kind 5: dst[K][RS][C4] = src[K][RS][C] with the channels zero-padded to C4 = the next multiple of 4 (the 3-channel stem filter)
 * blocks_per_job: workgroups per job (each job is a grid-stride loop; any count > 0 gives the same bits).  jobs_d NULL, njobs <= 0 or
 * blocks_per_job <= 0: HIFIHR_EINVAL, nothing written.  Every job's dst equals, bit for bit, what the separate entry it names writes. */
typedef struct hifihr_prep_job {
  const float* src;
  float* dst;
  int K, C, RS, kind;
} hifihr_prep_job;
int hifihr_weight_prep(const hifihr_prep_job* jobs_d, int njobs, int blocks_per_job, void* stream);

/* Name of the kernel a convolution of this shape runs on, as a profiler lists it: direction 0 forward, 1 backward-data (e.g.
 * "conv_halo_kernel", "bgemm_nt_rows_kernel<0>", "conv3x3_oc4_kernel", "conv_igemm_kernel"), 2 backward-weight (e.g.
 * "conv_halo_wgrad_kernel", "bgemm_tn_rows_kernel", "conv_wgrad_kernel").  The name comes from the same plan the launch reads
 * (csrc/conv.hip plan_conv / plan_wgrad).  This entry has no bias, activation, statistics or workspace arguments: it describes the
 * launch a caller makes with bias = stats = NULL, no activation, the workspace that hifihr_conv2d_workspace_bytes /
 * hifihr_conv2d_wgrad_workspace_bytes ask for, and the zero page present (i.e. not the first use inside a stream capture).
 * Measurement only. */
int hifihr_conv2d_describe(int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int direction, char* out, int cap);

/* conv2d_fwd that also accumulates the per-channel sum and sum of squares of y into stats_d (hifihr_bn_stats_floats(K)
 * floats, ALL ZERO on entry: see the self-cleaning rule below) from the accumulator registers, so the batch-norm that
 * follows needs no pass over y. */
int hifihr_conv2d_fwd_bnstats(const float* x_d, const float* w_d, float* y_d, float* stats_d, int N, int H, int W, int C, int K,
                              int R, int S, int stride, int pad, void* ws_d, size_t ws_bytes, void* stream);
/* Two convolutions of the SAME input in one launch (round 6): y1 = conv(x, w1; R1 x R1, pad1), y2 = conv(x, w2; R2 x R2, pad2), both with
 * `stride` and with their batch-norm statistics (stats1_d / stats2_d: the slot-buffer contract of hifihr_conv2d_fwd_bnstats) -- the strided
 * 3x3 convolution of a residual stage's first block and the 1x1 convolution of its downsample branch (torchvision BasicBlock.conv1 +
 * downsample[0], reference network/res_encoder.py:364-373), whose short 1x1 launch otherwise pays its start and end alone.  Results
 * identical to two hifihr_conv2d_fwd_bnstats calls.  _supported: both shapes run on the gathering row-share GEMM (C % 32 == 0,
 * K % 128 == 0, R in {1, 3}, stride 2). */
int hifihr_conv2d_fwd_bnstats_pair_supported(int N, int H, int W, int C, int stride, int K1, int R1, int pad1, int K2, int R2, int pad2);
int hifihr_conv2d_fwd_bnstats_pair(const float* x_d, const float* w1_d, float* y1_d, float* stats1_d, int K1, int R1, int pad1, const float* w2_d,
                                   float* y2_d, float* stats2_d, int K2, int R2, int pad2, int N, int H, int W, int C, int stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Train-mode BatchNorm2d fused with the residual add and ReLU of a ResNet BasicBlock, NHWC: x[M][C], M = N*H*W.
 * Replaces nn.BatchNorm2d(training=True) + `out += identity` + nn.ReLU and their autograd in the trunk
 * (reference network/res_encoder.py:364-373; vendored BasicBlock utils/Freihand_GNN_mano/network/resnet.py).
 * C % 4 == 0, C <= 4096.  act: 0 = none, 1 = ReLU, 2 = swish (x * sigmoid(x); MemoryEfficientSwish of the reference's
 * EfficientNet, network/efficientnet_pt/utils.py:36-52; no residual with swish).  stats_d / red_scratch_d hold hifihr_bn_stats_floats(C) floats: partial (sum, sum of
 * squares) over the M rows, spread over several slots to keep atomic contention low (from
 * hifihr_conv2d_fwd_bnstats, or hifihr_bn_stats for any other producer).  Since round 3 the FORWARD partials are float64
 * (double[32][2][C] at the start of the buffer, which must be 8-byte aligned): producers accumulate sums shifted by a value of their own
 * in fp32 and hand them over unshifted in fp64, the consumer forms mean and variance in fp64 -- the batch variance of a channel with
 * |mean| >> std is as good as a Welford pass (PyTorch's nn.BatchNorm2d), which `E[x^2] - mean^2` in fp32 was not.  The layout is private
 * to the library: callers only allocate, zero once, and pass the buffer along.
 * SELF-CLEANING: producers (hifihr_conv2d_fwd_bnstats, hifihr_dwconv2d_fwd, hifihr_wino_output_transform, hifihr_bn_stats,
 * the reduction inside hifihr_bn_act_bwd) ADD into stats_d / red_scratch_d, which must be all zero on entry;
 * hifihr_bn_act_fwd / hifihr_bn_act_bwd fold the slots inside their apply kernel (no separate finalize launch) and the
 * last workgroup of that kernel to finish -- elected through arrival counters stored behind the slots -- writes the zeros
 * back, so one zero-initialised buffer serves every step without a memset launch.  (Handed back zeroed: the slots and the arrival counters,
 * the first 128 C + 64 floats; the 2 C floats behind them are scratch of the wide-layer backward, written before they are read.)
 *   fwd: y = act( (x - mean) * invstd * gamma + beta + residual? ); writes save_mean/save_invstd[C] and updates
 *        running_mean/var (momentum, unbiased variance) when given (both or neither: one NULL is HIFIHR_EINVAL).
 *        M = 1 (nn.BatchNorm2d raises there) is defined: batch variance 0, save_invstd = 1 / sqrt(eps), y = act(beta + residual?), and
 *        running_var takes the BIASED value (0) -- the unbiased M / (M - 1) factor is applied for M > 1 only.  The same rule holds for
 *        hifihr_bn_finalize_fwd and the fused stem entry.
 *   bwd: g = dy * act'(z) (ReLU: y > 0 from y_d -- or, with y_d NULL and no residual input in the forward, the mask recomputed from x, needs beta_d; swish: z recomputed from x, needs beta_d); dx = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)); dres (may be NULL) = g;
 *        dgamma_acc[C] += sum g*xhat, dbeta_acc[C] += sum g (either may be NULL).
 * ---------------------------------------------------------------------------------------------- */
int hifihr_bn_stats_floats(int C);
int hifihr_bn_stats(const float* x_d, long M, int C, float* stats_d, void* stream);
int hifihr_bn_act_fwd(const float* x_d, float* stats_d /* consumed: zero on return */, const float* gamma_d, const float* beta_d,
                      const float* residual_d /* or NULL */, int act, long M, int C, float eps, float momentum, float* y_d,
                      float* save_mean_d, float* save_invstd_d, float* running_mean_d, float* running_var_d, void* stream);
/* Evaluation mode (module.eval(), reference train_hrnet.py:119-161): the same fused apply with the running statistics; nothing
 * is updated, no statistics buffer is involved. */
int hifihr_bn_act_eval(const float* x_d, const float* running_mean_d, const float* running_var_d, const float* gamma_d, const float* beta_d,
                       const float* residual_d /* or NULL */, int act, long M, int C, float eps, float* y_d, void* stream);
int hifihr_bn_act_bwd(const float* dy_d, const float* y_d /* act 1; NULL: recompute the mask (no-residual layers) */, const float* x_d, const float* save_mean_d,
                      const float* save_invstd_d, const float* gamma_d, const float* beta_d /* act 2 */, int act, long M, int C,
                      float* red_scratch_d, float* dx_d, float* dres_d, float* dgamma_acc_d, float* dbeta_acc_d, void* stream);

/* The ResNet stem, bn1 -> relu -> maxpool fused: pooled = MaxPool2d(3, 2, 1)(ReLU(BN(x))) on x[N][H][W][C] (reference: the
 * vendored trunk utils/Freihand_GNN_mano/network/resnet.py forward, `x = self.maxpool(self.relu(self.bn1(self.conv1(x))))`, driven
 * from network/res_encoder.py:364-373).  The full-resolution activation and its gradient never reach HBM: the forward reads the
 * nine taps of x through scale / shift / ReLU (tie rule of nn.MaxPool2d: first tap in scan order), the backward gathers the
 * pool's gradient from pooled_grad + tap on the fly inside the batch-norm reduction and apply kernels.  Same statistics-buffer
 * contract (all zero on entry, all zero on return) and the same save_mean / save_invstd / running-statistics outputs as
 * hifihr_bn_act_fwd; C % 4 == 0, C <= 512, H, W >= 2.  pooled_d [N][OH][OW][C], tap_d one byte per pooled element,
 * OH = (H - 1) / 2 + 1. */
int hifihr_bn_relu_maxpool_supported(int N, int H, int W, int C);
int hifihr_bn_relu_maxpool_fwd(const float* x_d, float* stats_d, const float* gamma_d, const float* beta_d, int N, int H, int W, int C,
                               float eps, float momentum, float* pooled_d, unsigned char* tap_d, float* save_mean_d, float* save_invstd_d,
                               float* running_mean_d, float* running_var_d, void* stream);
int hifihr_bn_relu_maxpool_bwd(const float* pooled_grad_d, const unsigned char* tap_d, const float* x_d, const float* save_mean_d,
                               const float* save_invstd_d, const float* gamma_d, const float* beta_d, int N, int H, int W, int C,
                               float* red_scratch_d, float* dx_d, float* dgamma_acc_d, float* dbeta_acc_d, void* stream);
/* The same backward with the forward's pooled OUTPUT handed back (pooled_d [N][OH][OW][C]): the batch-norm reduction then walks the pooled
 * grid -- the pool's gradient lives at the winning taps only and the winner's normalised value follows from the pooled value itself,
 * xhat = (z - beta) / gamma (channels with |gamma| < 1e-3 fetch the winner's x through tap_d) -- a quarter of the bytes of the pass over
 * every input pixel.  Results equal hifihr_bn_relu_maxpool_bwd's to the rounding of the sums. */
int hifihr_bn_relu_maxpool_bwd_y(const float* pooled_grad_d, const float* pooled_d, const unsigned char* tap_d, const float* x_d,
                                 const float* save_mean_d, const float* save_invstd_d, const float* gamma_d, const float* beta_d, int N, int H, int W,
                                 int C, float* red_scratch_d, float* dx_d, float* dgamma_acc_d, float* dbeta_acc_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depthwise convolution (groups == channels), NHWC fp32, k = 3 or 5, TensorFlow-style asymmetric zero padding.
 * Replaces the depthwise Conv2dStaticSamePadding of the reference's EfficientNet MBConv blocks
 * (reference network/efficientnet_pt/model.py:49-55,80; utils.py:122-145) and its autograd.
 * x[N][H][W][C], w[C][K][K] (= torch [C,1,K,K]), y[N][OH][OW][C]; stride 1 or 2; pad_top/pad_left explicit, bottom/right
 * implied by OH/OW:  pad_bottom = (OH - 1) * stride + K - H - pad_top (columns alike), the zero rows the last window needs below the
 * image.  Accepted: C % 4 == 0, 0 <= pad_top <= K - 1 and -(stride - 1) <= pad_bottom <= K - 1, i.e. y is
 * conv2d(F.pad(x, (pad_left, max(pad_right, 0), pad_top, max(pad_bottom, 0))), stride), OH = floor((H + pad_top + pad_bottom - K) / stride) + 1:
 * a negative pad_bottom down to -(stride - 1) is the row(s) a stride-2 floor division leaves unread (H + pads - K odd), not a crop.
 * Anything else -- an output smaller than the windows that fit (a crop), windows that lie in the padding alone, a pad of K or
 * more, OH <= 0 -- is HIFIHR_EINVAL with nothing written.  An input smaller than the filter is fine (H = 1, K = 5, pads 2 + 2).
 * bwd_data OVERWRITES dx.  bwd_weight ACCUMULATES into dw (fp32 atomics).  fwd: stats_d (may be NULL) = batch-norm slot buffer
 * (hifihr_bn_stats_floats(C) floats, all zero on entry, self-cleaning: see the batch-norm section) that receives the
 * per-channel sum / sum of squares of y, so the BatchNorm that follows needs no statistics pass.
 * ---------------------------------------------------------------------------------------------- */
int hifihr_dwconv2d_fwd(const float* x_d, const float* w_d, float* y_d, float* stats_d /* or NULL */, int N, int H, int W, int C,
                        int OH, int OW, int K, int stride, int pad_top, int pad_left, void* stream);
int hifihr_dwconv2d_bwd_data(const float* dy_d, const float* w_d, float* dx_d, int N, int H, int W, int C, int OH, int OW, int K,
                             int stride, int pad_top, int pad_left, void* stream);
int hifihr_dwconv2d_bwd_weight(const float* x_d, const float* dy_d, float* dw_d, int N, int H, int W, int C, int OH, int OW,
                               int K, int stride, int pad_top, int pad_left, void* stream);
/* The expand half of an MBConv block without its activated tensor (round 5): reference network/efficientnet_pt/model.py:73-80,
 *   x = swish(bn0(expand_conv(x)));  x = depthwise_conv(x)
 * x_d is the RAW output of the expand convolution; a = swish(x * gamma invstd + (beta - mean gamma invstd)) is formed as the depthwise
 * kernels load their rows (zero outside the image: the padding is of a) and never reaches HBM.  mean_d / invstd_d [C]: the batch
 * statistics of x (hifihr_bn_finalize_fwd below makes them from the convolution's slot buffer).  fwd: y, stats as hifihr_dwconv2d_fwd;
 * bwd_weight: dw += sum dy * a.  The gradient with respect to x is hifihr_dwconv2d_bwd_data followed by hifihr_bn_act_bwd(act = swish)
 * on (that, x): the batch-norm backward recomputes the activation's derivative from x alone. */
int hifihr_dwconv2d_fwd_bnswish(const float* x_d, const float* mean_d, const float* invstd_d, const float* gamma_d, const float* beta_d,
                                const float* w_d, float* y_d, float* stats_d /* or NULL */, int N, int H, int W, int C, int OH, int OW,
                                int K, int stride, int pad_top, int pad_left, void* stream);
int hifihr_dwconv2d_bwd_weight_bnswish(const float* x_d, const float* mean_d, const float* invstd_d, const float* gamma_d,
                                       const float* beta_d, const float* dy_d, float* dw_d, int N, int H, int W, int C, int OH, int OW,
                                       int K, int stride, int pad_top, int pad_left, void* stream);
/* The statistics half of a training-mode batch-norm on its own (what hifihr_bn_act_fwd does before it applies): the slot buffer of a
 * producer -> save_mean[C], save_invstd[C] (biased variance, eps inside the root), running statistics updated with `momentum`
 * (NULL: not kept), slots handed back all zero.  reference: nn.BatchNorm2d in training mode (model.py:73-76). */
int hifihr_bn_finalize_fwd(float* stats_d, long M, int C, float eps, float momentum, float* save_mean_d, float* save_invstd_d,
                           float* running_mean_d /* or NULL */, float* running_var_d /* or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pooling on NHWC fp32 activations (C % 4 == 0).
 * mmpool: MMPool((1,1)) of the reference encoder (network/res_encoder.py:247-265, called at :49):
 *   y[B][C] = max_hw(x) * w + mean_hw(x) * (1 - w), w = sigmoid(p_d[0]); x[B][HW][C].  fwd also writes argmax[B][C] (first
 *   maximum in scan order, like adaptive_max_pool2d), xmax[B][C], xavg[B][C] for the backward.
 *   bwd: dx[B][HW][C] (overwritten) and dp_acc_d[0] += d loss / d p (may be NULL).
 * maxpool2d: nn.MaxPool2d(k, s, p) for (k, s, p) = (3, 2, 1) (after the ResNet stem, network/res_encoder.py:345-373,
 *   torchvision resnet18.maxpool), (3, 1, 1) and (2, 2, 0) (LightEstimator, network/res_encoder.py:150-210):
 *   y[N][OH][OW][C], OH = (H + 2p - k)/s + 1; tap_d[N][OH][OW][C] bytes = winning tap (first maximum in scan order).
 *   bwd gathers: dx[N][H][W][C] is overwritten (no zero fill needed).
 * ---------------------------------------------------------------------------------------------- */
int hifihr_mmpool_fwd(const float* x_d, const float* p_d, int B, int HW, int C, float* y_d, int* argmax_d, float* xmax_d,
                      float* xavg_d, void* stream);
int hifihr_mmpool_bwd(const float* gy_d, const float* p_d, const int* argmax_d, const float* xmax_d, const float* xavg_d, int B,
                      int HW, int C, float* dx_d, float* dp_acc_d, void* stream);
int hifihr_maxpool2d_fwd(const float* x_d, int N, int H, int W, int C, int k, int s, int p, float* y_d, unsigned char* tap_d,
                         void* stream);
int hifihr_maxpool2d_bwd(const float* gy_d, const unsigned char* tap_d, int N, int H, int W, int C, int k, int s, int p,
                         float* dx_d, void* stream);
/* The same backward for a pool whose INPUT was a ReLU's output (VGG19: conv + ReLU -> MaxPool2d, reference utils/perceptual_loss.py:27-36
 * over torchvision's features): y_d = the pool's own output; a window's gradient passes only where y > 0, which IS the ReLU's backward at
 * the winning tap (the other taps receive nothing) -- dx_d is then the gradient of the convolution output, no pass over (dy, relu output)
 * of the four-times larger pre-pool tensor is needed. */
int hifihr_maxpool2d_bwd_relu(const float* gy_d, const unsigned char* tap_d, const float* y_d, int N, int H, int W, int C, int k, int s, int p,
                              float* dx_d, void* stream);
/* The pool whose output is FLATTENED next (LightEstimator: `base_layers(x).view(B, -1)` -> Linear, network/res_encoder.py:199-201): y_flat_d is
 * the [N][C * OH * OW] matrix in the reference's NCHW order, gy_flat_d its gradient; x / dx stay channels-last.  Saves the copy kernel a
 * reshape of the channels-last tensor costs in each direction. */
int hifihr_maxpool2d_fwd_flat(const float* x_d, int N, int H, int W, int C, int k, int s, int p, float* y_flat_d, unsigned char* tap_d,
                              void* stream);
int hifihr_maxpool2d_bwd_flat(const float* gy_flat_d, const unsigned char* tap_d, int N, int H, int W, int C, int k, int s, int p, float* dx_d,
                              void* stream);

/* normalize_batch_3C (reference network/res_encoder.py:212-216) fused with NCHW[B][3][H][W] -> NHWC4 [B][H][W][4]
 * (4th channel zero) for the first convolution. */
int hifihr_image_to_nhwc4(const float* images_d, float* out_d, int B, int H, int W, void* stream);
/* Same repack with an explicit zero border and optional normalisation: out[B][H + pt + pb][W + pl + pr][4].  Serves the
 * EfficientNet stem (reference network/efficientnet_pt/model.py:197-199: no input normalisation, Conv2dStaticSamePadding
 * k3 s2 pads (left 0, right 1, top 0, bottom 1)), which then runs on hifihr_conv2d_fwd with pad = 0. */
int hifihr_image_to_nhwc4_padded(const float* images_d, float* out_d, int B, int H, int W, int pad_top, int pad_left,
                                 int pad_bottom, int pad_right, int normalize, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LPIPS(net="alex"), version 0.1, the forward (csrc/lpips.hip; the backward follows in the next block).  Replaces `lpips.LPIPS(net="alex")` of the reference's
 * evaluation pass (built at train_hrnet.py:563, called at :158); the five convolutions of the AlexNet trunk
 * (torchvision features[0:12]) run on hifihr_conv2d_fwd with act = 1.  hifihr_amd/lpips.py is the caller.
 *
 * image_scale_to_nhwc4: the package's ScalingLayer fused with the repack the stem reads (train_hrnet.py:158,563):
 *   out[B][H][W][4] = ((images[B][3][H][W] - shift[c]) / scale[c], 0); shift3_host / scale3_host are HOST arrays of 3 floats
 *   (scale != 0).  One launch, true division.
 * maxpool2d_fwd_notap: nn.MaxPool2d(k, s, p) for inference, (k, s, p) = (3, 2, 0) only (the AlexNet pools, train_hrnet.py:158,563);
 *   y[N][OH][OW][C], OH = (H - 3)/2 + 1; no winning-tap bytes, no backward.  C % 4 == 0, H, W >= 3.  hifihr_maxpool2d_fwd
 *   keeps its own set {(3,2,1), (3,1,1), (2,2,0)}.
 * lpips_tap: one tap of the metric (train_hrnet.py:158,563: normalize_tensor, the squared difference, the tap's `lin` layer
 *   and spatial_average of the package) on two channels-last maps f0_d, f1_d [B][HW][C] -- e.g. the two halves of one [2B]
 *   batch -- and the 1x1 `lin` weights w_d[C] (no bias):
 *     n = f / (sqrt(sum_c f^2) + 1e-10),   val_d[b] = (accumulate ? val_d[b] : 0) + mean_pixels sum_c w_c (n0_c - n1_c)^2.
 *   Direct form (n0 - n1 per channel, never the expanded sums): identical maps give exactly 0.  Deterministic (fixed-order
 *   partial sums, no float atomics).  C % 4 == 0, 4 <= C <= hifihr_lpips_tap_max_channels() (512), B <= 65535; anything else
 *   is HIFIHR_EINVAL with val_d untouched.  partial_d: scratch of hifihr_lpips_tap_partial_floats(B) floats (any contents).
 * ---------------------------------------------------------------------------------------------- */
int hifihr_image_scale_to_nhwc4(const float* images_d, float* out_d, int B, int H, int W, const float* shift3_host,
                                const float* scale3_host, void* stream);
int hifihr_maxpool2d_fwd_notap(const float* x_d, int N, int H, int W, int C, int k, int s, int p, float* y_d, void* stream);
int hifihr_lpips_tap_max_channels(void);
size_t hifihr_lpips_tap_partial_floats(int B);
int hifihr_lpips_tap(const float* f0_d, const float* f1_d, const float* w_d, int B, int HW, int C, int accumulate, float* partial_d,
                     float* val_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LPIPS as a training loss: the backward of the three launches above (csrc/lpips.hip), gradient with respect to the FIRST image only --
 * the second is the target, a constant.  Not in the reference (its LPIPS is an evaluation metric, train_hrnet.py:158,563); the callers are
 * hifihr_amd/lpips.py LPIPS(differentiable=True) and the opt-in loss term `lpips` of hifihr_amd/losses.py.  The convolutions' backward is
 * hifihr_conv2d_bwd_data with the frozen weights on a gradient that lpips_tap_bwd_relu has already taken through the ReLU.  Every entry: no allocation, no synchronisation (capturable into
 * a hipGraph), no float atomics, every output element has ONE writer: the same bits on every call.
 *
 * lpips_tap_bwd: the gradient of one tap (hifihr_lpips_tap) with respect to f0_d; f1_d gets none.  Per pixel, eps = 1e-10:
 *     r0 = sqrt(sum_c f0_c^2), D0 = r0 + eps (r1, D1 alike);  n = f / D;  q_c = 2 w_c (n0_c - n1_c);  t = sum_c q_c f0_c
 *     d d / d f0_k = q_k / D0 - f0_k t / (r0 D0^2)     where r0 > 0
 *     d d / d f0_k = q_k / D0                          where r0 == 0  -- a CONVENTION: on an all-zero pixel the second numerator is 0;
 *                                                      torch autograd through sqrt gives NaN there
 *     gf0_d[b][p][k] = (accumulate ? gf0_d[b][p][k] : 0) + gval_d[b] / HW * d d / d f0_k
 *   gval_d[B]: the gradient arriving at val_d (device).  n0 - n1 is formed per channel exactly as the forward forms it: identical maps give
 *   a gradient of exactly 0.  The pixel -> (workgroup, lane group) mapping is the forward's, a function of (HW, C) alone.
 *   accepted:    C % 4 == 0, 4 <= C <= hifihr_lpips_tap_max_channels() (512), 1 <= B <= 65535, HW >= 1
 *   refused:     anything else, or a NULL f0_d / f1_d / w_d / gval_d / gf0_d: HIFIHR_EINVAL, gf0_d untouched
 *   overwritten: gf0_d with accumulate == 0; with accumulate != 0 it is read and added to (it must hold finite or intended values)
 * lpips_tap_bwd_relu: the same call for an f0_d that is a ReLU's output (every AlexNet tap): what it stores is the gradient of the ReLU's
 *   INPUT, gf0_d = ((accumulate ? gf0_d : 0) + gval_d[b] / HW * d d / d f0) * [f0 > 0] -- the mask covers the arriving gradient too.
 *   Bit for bit the unmasked call's result where f0 > 0, exactly 0 elsewhere (a NaN in f0 counts as not > 0).  Same accepted / refused /
 *   overwritten sets.  (hifihr_bias_relu_bwd serves C <= 256; the third tap has 384 channels.)
 * lpips_maxpool_fwd / lpips_maxpool_bwd: nn.MaxPool2d(3, 2), no padding, with a backward; x[N][H][W][C] -> y[N][OH][OW][C], OH = (H - 3)/2 + 1.
 *   TAPLESS design: the forward writes no winning-tap bytes (it is the kernel of hifihr_maxpool2d_fwd_notap); the backward recomputes each
 *   window's winner from the saved input x_d as a gather -- an input pixel looks at the at most 2 x 2 windows that cover it and adds the
 *   gy of those it wins, in ascending (oh, ow) order.  Tie rule = ATen's: the first maximum in row-major window order, found with the
 *   forward's (v > m) || isnan(v) scan from the first tap (a NaN wins, the last one of a window).
 *   accepted:    C % 4 == 0, C >= 4, H >= 3, W >= 3, N >= 1
 *   refused:     anything else or a NULL pointer: HIFIHR_EINVAL, y_d / dx_d untouched.  hifihr_maxpool2d_fwd / _bwd / _fwd_notap keep
 *                their own sets
 *   overwritten: y_d; dx_d[N][H][W][C] entirely -- rows and columns that no window covers (H or W even) get exactly 0
 * image_scale_to_nhwc4_bwd: the backward of hifihr_image_scale_to_nhwc4: gimg_d[B][3][H][W] = g4_d[B][H][W][c] / scale[c], the same
 *   true division as the forward; the fourth plane of g4_d is ignored.  scale3_host: HOST array of 3 floats.
 *   accepted:    B, H, W >= 1, scale[c] != 0
 *   refused:     anything else or a NULL pointer: HIFIHR_EINVAL, gimg_d untouched
 *   overwritten: gimg_d
 * ---------------------------------------------------------------------------------------------- */
int hifihr_lpips_tap_bwd(const float* f0_d, const float* f1_d, const float* w_d, const float* gval_d, int B, int HW, int C, int accumulate,
                         float* gf0_d, void* stream);
int hifihr_lpips_tap_bwd_relu(const float* f0_d, const float* f1_d, const float* w_d, const float* gval_d, int B, int HW, int C, int accumulate,
                              float* gf0_d, void* stream);
int hifihr_lpips_maxpool_fwd(const float* x_d, int N, int H, int W, int C, float* y_d, void* stream);
int hifihr_lpips_maxpool_bwd(const float* gy_d, const float* x_d, int N, int H, int W, int C, float* dx_d, void* stream);
int hifihr_image_scale_to_nhwc4_bwd(const float* g4_d, float* gimg_d, int B, int H, int W, const float* scale3_host, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused SSIM (11x11 gaussian window sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2, mean over all elements).
 * Replaces pytorch_ssim.ssim(img1, img2)   reference utils/pytorch_ssim/__init__.py:17-37,65-73
 * (called at reference losses.py:375 for the ssim_tex term) and its autograd w.r.t. img1.
 * img1/img2: [planes][H][W] with planes = B*C (contiguous NCHW); window11_h: the 11 normalised taps (HOST).
 * fwd writes one partial sum per tile (32x32; hifihr_ssim_partial_count of them): SSIM = sum(partial[0..hifihr_ssim_partial_count)) / (planes*H*W)
 * (summed by the caller; deterministic).  dA/dB/dC ([planes][H][W] each, all three or none) receive the
 * derivative maps the backward call consumes.  bwd: gimg1 = grad_out[0] * d mean(SSIM) / d img1; grad_out_d is
 * a DEVICE scalar (no host sync).
 * ---------------------------------------------------------------------------------------------- */
int hifihr_ssim_partial_count(int planes, int H, int W);
int hifihr_ssim_fwd(const float* window11_h, const float* img1_d, const float* img2_d, int planes, int H, int W,
                    float* partial_d, float* dA_d, float* dB_d, float* dC_d, void* stream);
int hifihr_ssim_bwd(const float* window11_h, const float* img1_d, const float* img2_d, const float* dA_d, const float* dB_d,
                    const float* dC_d, const float* grad_out_d, int planes, int H, int W, float* gimg1_d, void* stream);
/* The scalar glue of the call site in two more entry points (reference losses.py:375-377, `lambda * (1 - ssim)`):
 *   hifihr_ssim_finish: out_d[0] = offset + scale * sum(partial)   (SSIM: scale = 1 / n, offset = 0; the loss term: scale = -lambda / n,
 *                       offset = lambda) -- one launch, fixed summation order;
 *   hifihr_ssim_bwd_scaled: hifihr_ssim_bwd with the incoming gradient multiplied by out_scale (= -lambda for the loss term). */
int hifihr_ssim_finish(const float* partial_d, int count, float scale, float offset, float* out_d, void* stream);
int hifihr_ssim_bwd_scaled(const float* window11_h, const float* img1_d, const float* img2_d, const float* dA_d, const float* dB_d,
                           const float* dC_d, const float* grad_out_d, float out_scale, int planes, int H, int W, float* gimg1_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused training losses.  Replaces the torch-op evaluation of reference losses.py:226-453 (LossFunction.forward) and its
 * autograd for the terms below; every value comes back already multiplied by its lambda, as loss_dic holds it.
 *
 * geom_loss: out_d[5] = (joint_3d, vert_3d, edge_length, mshape, mpose)
 *   joint_3d / vert_3d = lambda * F.l1_loss or F.mse_loss (mse = 0 / 1: args.base_loss_fn, losses.py:259-266),
 *   edge_length = lambda * mean |edge(pred) - edge(gt)| over the 3 edges of every face (utils/losses_util.py:285-301),
 *   mshape / mpose = lambda * F.mse_loss(params, 0) (losses.py:398-406).
 *   joints[B][J][3], verts[B][V][3], shape[B][NS], pose[B][NP], faces_d[F][3] (F = 0 / NULL: no edge term);
 *   lambda5_h: HOST.  partial_d: B*5 floats of scratch.  bwd: gout_d[5] = gradient of each out element (DEVICE);
 *   vf_off_d[V+1] / vf_idx_d[3F] = vertex -> (face * 4 + corner) incidence lists in ascending face order (the edge
 *   gradient is gathered per vertex: deterministic, no atomics); any of gj/gv/gshape/gpose may be NULL.
 * photo_loss (the photometric block, losses.py:355-378, plus the `sil` term :388-390), from the renderer's rgba[B][4][H][W]:
 *   re_img_m = rgb * re_sil / 255 with re_sil = (alpha > 0 ? 255 : alpha); mask_rgbs = seg * imgs  (both written:
 *   the SSIM term consumes them); out_d[4] = (texture, mrgb, sil, mean(re_img_m) - mean(mask_rgbs)).
 *   seg_d: int64 [B][H][W] (segms_gt).  H*W % 4 == 0.  partial_d: hifihr_photo_loss_partial_floats() floats.
 *   bwd: grad_rgba[B][4][H][W] (overwritten; alpha channel 0: re_sil is detached in the reference) from gout_d[>=2]
 *   (texture, mrgb; may be NULL) and g_re_img_d (gradient arriving at re_img_m, e.g. from SSIM; may be NULL).
 * sil_post (models_res_nimble.py:219-220): re_sil[B][H][W] and maskRGBs[B][3][H][W] = images * (re_sil > 0) (may be NULL).
 *
 * What the contract tests pin (tests/test_hostsim_tail_contract.py):
 *   - every output of these entries is OVERWRITTEN, and every one is deterministic (fixed summation order, no float atomics): the same
 *     bits on a second call.  A term whose element count is 0 (F = 0, NS = 0, NP = 0, a joint set that is not given) is exactly 0.
 *   - zero lengths.  The edge term gives an edge whose PREDICTED length is exactly 0 no gradient (autograd: 0 / 0 = NaN); an edge whose
 *     gt length is 0 keeps the gradient of its predicted length.  sign(0) = 0: identical pred and gt give zero L1 gradients.  The bone
 *     terms use v / (|v| + 1e-4): at |v| = 0 the radial part of the gradient, vn (dn . v) / |v|, is taken as zero (autograd: NaN) and
 *     2 dn / 1e-4 remains.
 *   - NaN alpha.  re_sil = NaN at that pixel (NaN > 0 is false), re_img_m = NaN at that pixel only, mask_rgbs / maskRGBs = 0 there; all
 *     four photo_loss outputs are NaN; the backward reads out[3] = NaN, so EVERY rgb gradient is NaN (with gout_d NULL too: 0 x NaN) and the
 *     alpha channel stays exact zeros.
 *   - refused (HIFIHR_EINVAL, nothing launched or written): geom_loss: B / J / V <= 0, F / NS / NP < 0, F > 0 without faces, NS > 0 without
 *     shape, NP > 0 without pose, the backward with F > 0 and no vertex -> face tables, NULL partial / out / gout / lambda or a NULL
 *     joints / verts pointer.  joint_terms: J != 21, B <= 0, neither set given, a set without its gt, a gradient without its input, NULL
 *     out / gout / lambda.  photo_loss / sil_post: B / H / W <= 0, H * W % 4 != 0, a NULL pointer other than g_re_img_d / gout_d
 *     (sil_post: imgs_d may be NULL when mask_rgbs_d is).  loss_total: nparts outside 1 .. 4, a count outside 0 .. 64, a length below
 *     its count or above 64, a NULL pointer.  light_split: B <= 0, NULL lights / colors / directions / glights.
 * ---------------------------------------------------------------------------------------------- */
int hifihr_geom_loss_fwd(const float* joints_d, const float* joints_gt_d, const float* verts_d, const float* verts_gt_d,
                         const float* shape_d, const float* pose_d, const int32_t* faces_d, int B, int J, int V, int F, int NS,
                         int NP, int mse, const float* lambda5_h, float* partial_d, float* out_d, void* stream);
/* joint_2d, bone_direc, bone_direc_3d of LossFunction.__call__ (reference losses.py:267-282; bone_direction_loss of
 * utils/losses_util.py:217-283 with confidence 1) in ONE launch per direction: j2d / j2d_gt [B][21][2] (or both NULL), joints /
 * joints_gt [B][21][3] (or both NULL); lam3_host = (lambda_j2d_gt, lambda_bone_direc, lambda_bone_direc_3d), host memory; out3_d =
 * the three lambda-weighted terms (a term whose inputs are NULL is 0).  bwd: g_j2d_d / g_joints_d (either may be NULL) = gradient of
 * sum_k gout3_d[k] out3[k]. */
int hifihr_joint_terms_fwd(const float* j2d_d, const float* j2d_gt_d, const float* joints_d, const float* joints_gt_d, int B, int J, int mse,
                           const float* lam3_host, float* out3_d, void* stream);
int hifihr_joint_terms_bwd(const float* j2d_d, const float* j2d_gt_d, const float* joints_d, const float* joints_gt_d, int B, int J, int mse,
                           const float* lam3_host, const float* gout3_d, float* g_j2d_d, float* g_joints_d, void* stream);
/* open_2dj, open_bone_direc, open_2dj_de: the self-supervised keypoint terms of the reference's deprecated loss_func (losses.py:45-63,
 * 79-85; bone_direction_loss of utils/losses_util.py:217-283 WITH the detector's confidences) in ONE launch per direction.
 * j2d / open_2dj [B][21][2] in pixels, open_2dj_con [B][21] (or [B][21][1]: the same memory), lam3_host = (lambda_j2d, lambda_bone_direc,
 * lambda_j2d_de) in host memory (0 = the term is not requested).  out3_d:
 *   out[0] = lam0 sum_bj rho(d_bj) (c_bj w_j)^2 / sum_bj (c_bj w_j)^2 with d = |j2d - open_2dj|, rho(d) = d^2 / 10 for d < 5, d - 2.5
 *            otherwise, w = (2, 1, 1, 1, 1.5, 1, 1, 1, 1.5, 1, 1, 1, 1.5, 1, 1, 1, 1.5, 1, 1, 1, 1.5); both sums run over the whole batch
 *   out[1] = lam1 mean over the B x 20 bones of |vn - von|^2 c_parent c_child, unit bone vectors v / (|v| + 1e-4)
 *   out[2] = lam2 mean (open_2dj - j2d)^2 (always MSE, as in the reference)
 * bwd: g_j2d_d [B][21][2] = gradient of sum_k gout3_d[k] out3[k] (overwritten).  No gradient goes to the detections or the confidences.
 * Decided corners:
 *   - d = 0: the gradient of rho is (j2d - open_2dj) / 5 for d < 5, so exactly 0 there (autograd of the reference: sqrt'(0) x 0 = NaN);
 *     value and slope of rho agree at d = 5, so the branch taken at the boundary does not matter.  Coincident joints (|v| = 0): as for
 *     the bone terms of joint_terms above.
 *   - a batch whose weights (c w)^2 sum to 0: out[0] = 0 and its gradient is 0, exactly.  A DELIBERATE departure: the reference computes
 *     0 / 0 = NaN there.  (out[1] is 0 as well: every bone's confidence is 0.)
 * Both directions are deterministic (one workgroup forward with a fixed summation order; one thread per sample backward, no atomics):
 * the same bits on a second call.  Nothing is allocated or synchronised.
 * Refused (HIFIHR_EINVAL, nothing launched or written): J != 21, B <= 0, a NULL pointer. */
int hifihr_open2d_terms_fwd(const float* j2d_d, const float* open_2dj_d, const float* open_2dj_con_d, int B, int J, const float* lam3_host,
                            float* out3_d, void* stream);
int hifihr_open2d_terms_bwd(const float* j2d_d, const float* open_2dj_d, const float* open_2dj_con_d, int B, int J, const float* lam3_host,
                            const float* gout3_d, float* g_j2d_d, void* stream);
int hifihr_geom_loss_bwd(const float* joints_d, const float* joints_gt_d, const float* verts_d, const float* verts_gt_d,
                         const float* shape_d, const float* pose_d, const int32_t* faces_d, const int32_t* vf_off_d,
                         const int32_t* vf_idx_d, int B, int J, int V, int F, int NS, int NP, int mse, const float* lambda5_h,
                         const float* gout_d, float* gj_d, float* gv_d, float* gshape_d, float* gpose_d, void* stream);
int hifihr_photo_loss_partial_floats(void);
int hifihr_photo_loss_fwd(const float* rgba_d, const float* imgs_d, const int64_t* seg_d, int B, int H, int W, float l_tex,
                          float l_mrgb, float l_sil, float* re_img_m_d, float* mask_rgbs_d, float* partial_d, float* out_d,
                          void* stream);
int hifihr_photo_loss_bwd(const float* rgba_d, const float* re_img_m_d, const float* mask_rgbs_d, const float* g_re_img_d,
                          const float* gout_d, const float* fwd_out_d, int B, int H, int W, float l_tex, float l_mrgb,
                          float* grad_rgba_d, void* stream);
int hifihr_sil_post(const float* rgba_d, const float* imgs_d, int B, int H, int W, float* re_sil_d, float* mask_rgbs_d,
                    void* stream);
/* loss = sum of the selected terms (reference train_hrnet.py:98-104: the sum over args.losses of loss_dic) when the terms are entries of
 * the fused loss kernels' small output vectors: total_d[0] = sum_i sum_{j < counts[i]} parts[i][j], parts in order (fixed summation
 * order); nparts <= 4, counts <= 64.  `parts` / `grads` are HOST arrays of DEVICE pointers.
 * bwd: grads[i][j] = gtotal_d[0] for j < counts[i], 0 for counts[i] <= j < lengths[i] (the vectors' full lengths). */
int hifihr_loss_total_fwd(const float* const* parts, const int* counts, int nparts, float* total_d, void* stream);
int hifihr_loss_total_bwd(const float* gtotal_d, float* const* grads, const int* counts, const int* lengths, int nparts,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * Small-batch fully connected layer of the regression heads: y[B][O] = act( BN1d?( x[B][I] W[O][I]^T + b ) ).
 * Replaces nn.Linear (+ nn.BatchNorm1d, training mode) (+ nn.ReLU) and their autograd in the reference's HandEncoder /
 * LightEstimator heads (reference network/res_encoder.py:52-145, 150-210).  Any I (16-byte loads when I % 4 == 0); act 0 = none, 1 = ReLU,
 * 2 = swish (z_d receives the pre-activation, needed by the backward), 3 = sigmoid -- 2 / 3 serve the squeeze-excite
 * layers below and take no batch-norm.
 * Batch-norm (gamma_d != NULL, B <= 64): batch statistics over the B rows, running statistics updated with `momentum`
 * (unbiased variance), z_d[B][O] receives the pre-normalisation output, save_mean_d / save_invstd_d[O] the statistics.
 * bwd: dy_d = gradient of y; y_d (act 1) gives the ReLU mask; dz_scratch_d[B][O]; dW_acc_d[O][I], db_acc_d[O],
 *      dgamma_acc_d[O], dbeta_acc_d[O] ACCUMULATE (pass the gradient buffers); dx_d[B][I] is overwritten (NULL: skipped).
 * The contract of these entries (tests/test_hostsim_gemm_contract.py):
 *   - B, I, O > 0 (any values), act 0..3, non-null x, w, y (fwd) / dy, x, w (bwd); act 1 / 3 need y_d and act 2 needs z_d in the backward,
 *     act 2 needs z_d in the forward, dx_d needs dz_scratch_d.  Batch-norm: B <= 64, act 0 / 1 only (both directions), beta, z, save_mean,
 *     save_invstd given, running_mean_d and running_var_d both or neither.  Anything else: HIFIHR_EINVAL, nothing written.
 *   - z_d is written only with batch-norm or act 2, save_mean_d / save_invstd_d only with batch-norm, the running statistics only when given.
 *   - B = 1 with batch-norm (nn.BatchNorm1d raises): the hifihr_bn_* rule for M = 1 -- variance 0, save_invstd = 1 / sqrt(eps),
 *     y = act(beta) to rounding, the running variance takes the BIASED value (0), dz and so dW, dx vanish.
 *   - two calls give the same bits, EXCEPT dx_d at O > 64: it is summed over 64-feature splits of O with fp32 atomics (equal up to their order).
 * ---------------------------------------------------------------------------------------------- */
int hifihr_linear_fwd(const float* x_d, const float* w_d, const float* b_d /* or NULL */, int B, int I, int O, int act,
                      const float* gamma_d /* or NULL: no batch-norm */, const float* beta_d, float eps, float momentum,
                      float* running_mean_d, float* running_var_d, float* y_d, float* z_d, float* save_mean_d,
                      float* save_invstd_d, void* stream);
int hifihr_linear_bwd(const float* dy_d, const float* y_d, const float* x_d, const float* w_d, int B, int I, int O, int act,
                      const float* gamma_d, const float* z_d, const float* save_mean_d, const float* save_invstd_d,
                      float* dz_scratch_d, float* dW_acc_d, float* db_acc_d, float* dgamma_acc_d, float* dbeta_acc_d,
                      float* dx_d, void* stream);

/* Grouped launches for independent layers of the same depth (the HandEncoder's five to six heads, reference
 * network/res_encoder.py:112-131, 146-160): up to 6 members per call, no batch-norm, act 0 / 1; one launch forward, two backward
 * instead of one / two PER LAYER (each is a latency-bound ~8 us kernel on 8-32 workgroups).  `descs` is a HOST array.
 * bwd members: dy, y (act 1), dz_scratch[B][O] required; dW_acc / db_acc accumulate (NULL: skipped); dx overwritten (NULL: skipped).
 * n outside 1..6, a member with act 2 / 3, a null x / w / y or a size <= 0: HIFIHR_EINVAL, nothing written.  Members may differ in B, I, O;
 * every member's results are bit-identical to its single launch (dx at O > 64: up to the order of its atomics). */
typedef struct hifihr_linear_desc {
  const float *x, *w, *b; /* b may be NULL */
  float* y;
  int B, I, O, act;
  const float* dy;
  float *dz_scratch, *dW_acc, *db_acc, *dx;
} hifihr_linear_desc;
int hifihr_linear_fwd_group(const hifihr_linear_desc* descs, int n, void* stream);
int hifihr_linear_bwd_group(const hifihr_linear_desc* descs, int n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Squeeze-and-excitation of the EfficientNet MBConv block (reference network/efficientnet_pt/model.py:82-86):
 *   y = x * sigmoid( W2 swish( W1 mean_hw(x) + b1 ) + b2 ),  x[B][HW][C] NHWC, C % 4 == 0.
 * se_pool: mean_d[B][C] += mean over HW (mean_d must be ZERO on entry: partial sums are added with atomics).
 * The two layers are hifihr_linear_fwd / _bwd with act 2 and 3.  se_scale: y = x * gate[b][c] (+ add[b][c] * add_scale when
 * add_d != NULL).  Backward: se_bwd_gate: dgate_d[B][C] += sum_hw dy * x (zero on entry); then the linear backwards give
 * dmean; finally dx = se_scale(dy, gate, add = dmean, add_scale = 1 / HW) folds the pooling branch into the same pass.
 * ---------------------------------------------------------------------------------------------- */
int hifihr_se_pool(const float* x_d, int B, int HW, int C, float* mean_zeroed_d, void* stream);
int hifihr_se_scale(const float* x_d, const float* gate_d, const float* add_d /* or NULL */, float add_scale, int B, int HW, int C,
                    float* y_d, void* stream);
int hifihr_se_bwd_gate(const float* dy_d, const float* x_d, int B, int HW, int C, float* dgate_zeroed_d, void* stream);
/* The two layers as ONE launch forward and TWO backward (round 4; replaces the four hifihr_linear_* calls per block and direction of
 * reference network/efficientnet_pt/model.py:83-86).  w1_d[SQ][C], w2t_d[SQ][C] = the TRANSPOSE of the expand weight W2[C][SQ]
 * (hifihr_weight_prep kind 0 provides it once per step), C % 4 == 0, C <= 4096, SQ <= 256 (hifihr_se_mlp_supported).
 * fwd: reads the pooled means from mean_acc_d[B][C] (what hifihr_se_pool accumulated) and hands that buffer back ZEROED; writes
 *      mean_d[B][C], z1_d[B][SQ] (pre-activation), h1_d[B][SQ] = swish(z1), gate_d[B][C] = sigmoid(h1 W2^T + b2).
 * bwd: reads dgate_acc_d[B][C] (hifihr_se_bwd_gate's sums; handed back ZEROED); writes dz2_d[B][C], dz1_d[B][SQ] (scratch) and
 *      dmean_d[B][C]; ACCUMULATES (+=) dW1[SQ][C], db1[SQ], dW2[C][SQ], db2[C] -- each element summed over the batch by one thread in a
 *      fixed order (bit-reproducible). */
int hifihr_se_mlp_supported(int C, int SQ);
/* Drop-connect + skip connection of an MBConv block in one pass (reference network/efficientnet_pt/utils.py:82-91 `drop_connect`,
 * model.py:91-94): out_d = x_d / keep * floor(keep + u_d[b]) (+ skip_d when not NULL); x / skip / out [B][per_sample], per_sample % 4 == 0,
 * u_d[B] the per-sample uniform draws.  The backward is the same call on dy with skip_d = NULL. */
int hifihr_drop_connect_add(const float* x_d, const float* skip_d /* or NULL */, const float* u_d, float keep, int B, size_t per_sample,
                            float* out_d, void* stream);
int hifihr_se_mlp_fwd(float* mean_acc_d, const float* w1_d, const float* b1_d, const float* w2t_d, const float* b2_d, int B, int C, int SQ,
                      float* mean_d, float* z1_d, float* h1_d, float* gate_d, void* stream);
int hifihr_se_mlp_bwd(float* dgate_acc_d, const float* gate_d, const float* z1_d, const float* h1_d, const float* mean_d, const float* w1_d,
                      const float* w2t_d, int B, int C, int SQ, float* dz2_d, float* dz1_d, float* dmean_d, float* dw1_acc_d, float* db1_acc_d,
                      float* dw2_acc_d, float* db2_acc_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation: Procrustes-with-scale alignment of pred_d[B][N][3] to gt_d[B][N][3] and the
 * aligned error, one workgroup per sample, fp64 inside.  Replaces the per-sample numpy loop of reference
 * train_hrnet.py:227-243 over utils/train_utils.py:267-290 (align_w_scale: centre, Frobenius-normalise,
 * scipy.linalg.orthogonal_procrustes -- no determinant correction --, apply).
 *   aligned_d[B][N][3] (or NULL) = the aligned prediction;  err_sum_d[B] = sum_n || aligned_n - gt_n ||_2
 * (MPJPE / MPVPE = sum_b err_sum_d[b] / (B N), in the unit of the inputs).
 * The rotation is the orthogonal polar factor R = U V^T of M = A^T B = U diag(w) V^T (A, B the centred, normalised gt and pred), from
 * a singular value decomposition of M itself, as scipy takes it: a direction whose singular value vanishes is KEPT.
 * Rank-deficient input (a set that is coplanar, collinear or a single point, N <= 3 included): R is then not unique -- LAPACK returns
 * some orthonormal completion, scipy uses that one; this entry completes with the proper rotation (det R = +1) -- and aligned_d may
 * differ from scipy's by the freedom: a reflection through the plane, a rotation about the line.  When only pred is degenerate the
 * freedom acts on nothing and aligned_d is unique.  The distances || aligned_n - gt_n || and err_sum_d do not depend on the choice
 * and equal scipy's.  A singular value down to 1e-12 of the largest still decides R (the points are read as fp32, everything after
 * is fp64); below 1e-14 it counts as zero.  N = 1, or gt a single repeated point: scale 0, aligned_n = mean(gt).
 * Deterministic: a second call gives the same bits, and err_sum_d is the same bits with aligned_d NULL or given.
 * Refused (HIFIHR_EINVAL, nothing launched or written): B <= 0, N <= 0, pred_d / gt_d / err_sum_d NULL.
 * ---------------------------------------------------------------------------------------------- */
int hifihr_procrustes_error(const float* pred_d, const float* gt_d, int B, int N, float* aligned_d /* or NULL */,
                            float* err_sum_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Benchmark metrics: the counts behind the FreiHAND benchmark's PCK / AUC (reference utils/fh_utils.py:719-815, EvalUtil) and
 * F-score (the benchmark's calculate_fscore).  The device counts; hifihr_amd/evaluate.py (pck_auc, fscore) turns the counts into
 * curves, areas and scores in float64 on the host.
 *
 * hifihr_point_error_hist: per-keypoint histogram of d = || pred - gt ||_2 over the visible samples, one launch.
 *   pred_d / gt_d [n][K][3] fp32;  vis_d [n][K] uint8 (non-zero = visible) or NULL = all visible;
 *   thr_h[T]: HOST array of doubles, finite and strictly increasing, 1 <= T <= 128; it is copied into the kernel's arguments (the
 *   caller may free it on return) and never re-derived on the device -- the thresholds compared are the caller's bits.
 *   hist_d[K][T + 1] int32: hist[k][t] = #{ thr[t-1] < d <= thr[t] } (thr[-1] = -inf), hist[k][T] = #{ d > thr[T-1] or d not a number };
 *     the comparison is <=, as in EvalUtil._get_pck: pck[k][t] = sum(hist[k][0..t]) / sum(hist[k][0..T]).
 *   sum_d[K] double = sum of d over the visible samples of the keypoint (not a number when one d is).
 *   d is the fp64 square root of (dx dx + dy dy) + dz dz, the differences taken in fp64 from the widened fp32 coordinates (exact).
 * Every element of hist_d and sum_d is written (a keypoint without a visible sample: zeros); the caller clears nothing.
 * Deterministic: a second call gives the same bits, sum_d included (a fixed summation order).
 * Refused (HIFIHR_EINVAL, nothing launched or written): pred_d / gt_d / thr_h / hist_d / sum_d NULL, n / K / T <= 0, T > 128, a
 * threshold that is not finite or not greater than its predecessor.
 *
 * hifihr_fscore_counts: two-sided nearest-neighbour counts between the point sets of each sample, one memset and one launch.
 *   pred_d [B][Np][3], gt_d [B][Ng][3] fp32 (any Np, Ng: the searched set passes through LDS in tiles);
 *   thr_h[T]: HOST array of doubles, finite and > 0 (any order), 1 <= T <= 8, copied like the above;
 *   counts_d[B][2][T] int32: counts[b][0][t] = #{ predicted points whose nearest ground-truth point is at distance < thr[t] }
 *     (the precision numerator, of Np), counts[b][1][t] = the same from ground truth to prediction (the recall numerator, of Ng).
 *   The comparison is sqrt(min d^2) < thr, STRICT, as in calculate_fscore; d^2 = (dx dx + dy dy) + dz dz in fp64 as above.
 *   A pair whose d^2 is not a number is skipped; a point all of whose pairs are is not counted.
 * Every element of counts_d is written; deterministic (integer sums, a minimum).
 * Refused (HIFIHR_EINVAL, nothing launched or written): pred_d / gt_d / thr_h / counts_d NULL, B / Np / Ng / T <= 0, T > 8, a threshold
 * that is not finite or not > 0, 2 B ceil(max(Np, Ng) / 64) >= 2^31 (the grid).
 * ---------------------------------------------------------------------------------------------- */
int hifihr_point_error_hist(const float* pred_d, const float* gt_d, const uint8_t* vis_d /* or NULL */, int n, int K, const double* thr_h,
                            int T, int32_t* hist_d, double* sum_d, void* stream);
int hifihr_fscore_counts(const float* pred_d, const float* gt_d, int B, int Np, int Ng, const double* thr_h, int T, int32_t* counts_d,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * FreiHAND training augmentation: gathers B samples from a uint8 dataset cache resident in
 * device memory and applies the reference's nearest-neighbour affine warp (reference data/dataset.py:223-270,
 * utils/handutils.py:48-60 = PIL Image.transform(AFFINE), zero fill) + to_tensor (+ torch.round for masks).
 *   img_rgbx_d[n][H][W]   uint32, bytes R, G, B, X     mask_d[n][H][W] uint8 (0 / 255)
 *   idx_d[B]              sample indices into the cache
 *   coef_fix_d[B][6]      PIL's 16.16 fixed-point terms of the six AFFINE coefficients (a b c; d e f):
 *                         {FIX(a), FIX(b), FIX(c + a/2 + b/2), FIX(d), FIX(e), FIX(f + d/2 + e/2)}, FIX(v) = floor(v * 65536 + 0.5)
 *   out_img_d[B][3][H][W] = u8 / 255,  out_mask_d[B][3][H][W] = round(u8 / 255) repeated over 3 channels (either may be NULL)
 * Bit-exact with PIL for the same coefficients.
 * Refused (HIFIHR_EINVAL, nothing launched): B / H / W <= 0, H * W >= 2^24 (the kernels index a plane with 32-bit integers scaled by
 * 16.16 terms; hifihr_freihand_batch and _batch_step refuse the same), idx_d / coef_fix_d NULL, both outputs NULL, an output given
 * without its source.
 * ---------------------------------------------------------------------------------------------- */
int hifihr_freihand_augment(const uint32_t* img_rgbx_d, const uint8_t* mask_d, const int* idx_d, const int* coef_fix_d, int B, int H,
                            int W, float* out_img_d, float* out_mask_d, void* stream);

/* One FreiHAND training batch in two launches: the warp above (plus segms = mask channel 0 as int64, the reference's
 * `masks[:, 0].long()`, utils/traineval_util.py:104) and everything else the sample dict and data_dic hold
 * (reference data/dataset.py:256-275 per sample, utils/traineval_util.py:21-111 per batch):
 *   Ks = post_rot_trans . K[idx];  joints / verts = (R p^T)^T;  Ps = [Ks | 0];  j2d_gt = (Ks j)_xy / (Ks j)_z (fh_utils.py:30-39);
 *   scales[idx];  idxs as int64.
 * Cache (device): Ks_d[n][3][3], joints_d[n][J][3], verts_d[n][V][3], scales_d[n].
 * packed_d[25 B] int32, ONE host-to-device copy per batch: idx[B], coef_fix[B][6], post_rot_trans[B][3][3] (float bits),
 * rot_mat[B][3][3] (float bits).  Every output may be NULL.  Outputs: out_Ks[B][3][3], out_Ps[B][3][4], out_joints[B][J][3],
 * out_verts[B][V][3], out_j2d[B][J][2], out_scales[B], out_idxs[B] (int64), out_segm[B][H][W] (int64).
 * J = 0 / V = 0 are accepted (joints_d / verts_d may then be NULL).  Refused (HIFIHR_EINVAL, nothing launched or written), by this entry
 * and by hifihr_freihand_batch_step: B / H / W <= 0, H * W >= 2^24, J / V < 0, NULL img / mask / Ks / scales / packed, J > 0 without
 * joints_d, V > 0 without verts_d. */
int hifihr_freihand_batch(const uint32_t* img_rgbx_d, const uint8_t* mask_d, const float* Ks_d, const float* joints_d, const float* verts_d,
                          const float* scales_d, int J, int V, const int* packed_d, int B, int H, int W, float* out_img_d,
                          float* out_mask_d, long long* out_segm_d, float* out_Ks_d, float* out_Ps_d, float* out_joints_d,
                          float* out_verts_d, float* out_j2d_d, float* out_scales_d, long long* out_idxs_d, void* stream);
/* The same two launches, which additionally emit what every training iteration derives from the batch before the model runs
 * (reference train_hrnet.py:62-68: root_xyz = joints[:, ROOT]; joints -= root; verts -= root;  models_res_nimble.py:184-186,228-235:
 * the NDC camera terms of PerspectiveCameras(focal_length=-fcl, principal_point=prp)):
 *   out_root[B][3] = joints[:, root_id] (root_id < 0: zeros), out_joints_rel[B][J][3], out_verts_rel[B][V][3],
 *   out_cam_ndc[B][4] = (-2 fx / s, -2 fy / s, 1 - 2 cx / s, 1 - 2 cy / s) with s = image_size, from out_Ks.  Any may be NULL.
 * The ten outputs shared with hifihr_freihand_batch are the same bits.  Also refused: root_id >= J, image_size <= 0 or NaN. */
int hifihr_freihand_batch_step(const uint32_t* img_rgbx_d, const uint8_t* mask_d, const float* Ks_d, const float* joints_d,
                               const float* verts_d, const float* scales_d, int J, int V, const int* packed_d, int B, int H, int W,
                               float* out_img_d, float* out_mask_d, long long* out_segm_d, float* out_Ks_d, float* out_Ps_d,
                               float* out_joints_d, float* out_verts_d, float* out_j2d_d, float* out_scales_d, long long* out_idxs_d,
                               int root_id, float image_size, float* out_root_d, float* out_joints_rel_d, float* out_verts_rel_d,
                               float* out_cam_ndc_d, void* stream);
/* The 2-D detections of the same batch, for the self-supervised keypoint terms (hifihr_open2d_terms_*) and the `*_self` photometric
 * terms: ONE more launch behind hifihr_freihand_batch (reference data/dataset.py:196-201, 255-257; utils/traineval_util.py:55-66, 106-111).
 * Cache (device): open_2dj_d[n][21][2] in pixels of the stored image, open_2dj_con_d[n][21].  idx_d[B] (the first B words of packed_d),
 * total_d[B][3][3]: the float32 forward affine of each sample's image warp (hifihr_amd.data.batch_affine_terms).  Outputs, any may be NULL
 * but not all:
 *   out_open_2dj_d[B][21][2] = total . (x, y, 1), each coordinate as fmaf(t0, x, fmaf(t1, y, t2)): handutils.transform_coords WITHOUT its
 *                              final truncation to integers (a deliberate departure: the sub-pixel position is kept)
 *   out_con_d[B][21]         = the cached confidences, bit for bit
 *   out_texture_con_d[B]     = mean_j([min_j con > 0.1] con_j) x ([idx < 32560] + 0.1), summed in joint order, from the confidences
 *                              BEFORE the mix below
 * semi_below > 0 (= ceil(32560 semi_ratio); needs j2d_gt_d[B][21][2], the batch's own out_j2d): a sample with idx % 32560 < semi_below
 * takes j2d_gt for its detections and 1 for its confidences.  0: no mix.
 * An index outside 0 .. n - 1 gives that sample zeros (the indices live in device memory: the entry cannot refuse them).
 * Refused (HIFIHR_EINVAL, nothing launched or written): n / B <= 0, semi_below < 0, semi_below > 0 without j2d_gt_d, NULL open_2dj_d /
 * open_2dj_con_d / idx_d / total_d, every output NULL. */
int hifihr_freihand_keypoints(const float* open_2dj_d, const float* open_2dj_con_d, int n, const int* idx_d, const float* total_d,
                              const float* j2d_gt_d, int semi_below, int B, float* out_open_2dj_d, float* out_con_d,
                              float* out_texture_con_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * HO-3D training sample assembly (the HO-3D half): the hand crop of reference data/dataset.py:1105-1215.
 * Frames live in device memory as for FreiHAND (img_rgbx_d[n][FH][FW] uint32 R,G,B,X; hand_mask_d[n][FH][FW] uint8 = channel 0 of the
 * reference's mask image); the host computes each sample's crop window from its projected joints (hifihr_amd/data.py:ho3d_crop_windows,
 * the reference's float32 arithmetic) and ships ONE packed int32 buffer per batch:
 *   packed_d[8 B]: idx[B], box[B][4] = the crop box (x0, y0, x1, y1) rounded as Pillow's Image.crop rounds it (half to even),
 *                  window[B][3] = crop centre u, v and scale (float bits)
 * Three launches: the resampling tables of Pillow's Image.resize (libImaging/Resample.c, evaluated in double on the device), the
 * crop + resize of frame (bilinear) and hand mask (bicubic) = torchvision's resized_crop on PIL images, and the small tensors:
 *   out_img_d[B][3][S][S] = u8 / 255 (`img_crop`), out_mask_d[B][1][S][S] = round(u8 / 255) (`hand_mask_crop`), S = out_size (224),
 *   out_K_d[B][3][3] = T . S . K (`K_crop`, :1206-1210), out_uv21_d[B][21][2] = (uv21 - centre) * scale + S / 2 (`uv21_crop`, :1186-1188),
 *   out_xyz21_d[B][21][3] = xyz21[idx].  Any output may be NULL.  Pixels bit-exact with Pillow (tests/golden/ho3d_path.npz).
 * ws_d: hifihr_ho3d_workspace_bytes(B, out_size) bytes of scratch (any contents).
 * Bit-exact for every box up to HIFIHR_HO3D_MAX_WINDOW = 800 pixels on an edge at every out_size in 1 .. 256, whatever the number of
 * filter taps that takes (800 -> 16: 200 per output pixel and axis; the workspace is sized for it).  800 is the most ho3d_crop_windows can
 * produce at any inp_res (640 / 0.8).  The boxes live in device memory, so the entry cannot refuse one: a box that is longer than
 * that on either edge, EMPTY or INVERTED (x1 <= x0 or y1 <= y0; Pillow raises) gives that sample's out_img_d and out_mask_d as all
 * zeros; the small outputs do not depend on the box.  hifihr_amd.data.HO3DDeviceCache.batch raises on the host for such a window.
 * Refused (HIFIHR_EINVAL, nothing launched or written): B / FH / FW <= 0, out_size outside 1 .. 256, packed_d or ws_d NULL, ws_bytes
 * below hifihr_ho3d_workspace_bytes(B, out_size) (which returns 0 for a refused B / out_size), an output given without its source.
 * ---------------------------------------------------------------------------------------------- */
#define HIFIHR_HO3D_MAX_WINDOW 800
size_t hifihr_ho3d_workspace_bytes(int B, int out_size);
int hifihr_ho3d_batch(const uint32_t* img_rgbx_d, const uint8_t* hand_mask_d, const float* Ks_d, const float* uv21_d, const float* xyz21_d,
                      int FH, int FW, const int* packed_d, int B, int out_size, void* ws_d, size_t ws_bytes, float* out_img_d,
                      float* out_mask_d, float* out_K_d, float* out_uv21_d, float* out_xyz21_d, void* stream);
/* What the HO-3D loader returns besides the crop (reference data/dataset.py:1023-1215: open_2dj_crop, open_2dj_con, depth_crop), each ONE
 * more launch behind hifihr_ho3d_batch that reads idx, box and window from the SAME packed_d: no further staged copy.
 *
 * hifihr_ho3d_keypoints: the 2-D detections through the crop window (:1199-1203).
 *   Cache (device): open_2dj_d[n][21][2] in pixels of the stored frame (FreiHAND joint order), open_2dj_con_d[n][21].
 *   out_open_2dj_d[B][21][2] = (open_2dj[idx] - centre) * scale + out_size / 2 (the integer quotient, as a float): a subtraction, a product
 *                              and a sum, each rounded to float32, the arithmetic of out_uv21_d above -- detections equal to uv21 give
 *                              out_uv21_d's bits
 *   out_con_d[B][21]         = the cached confidences, bit for bit
 *   An index outside 0 .. n - 1 gives that sample zeros (the indices live in device memory: the entry cannot refuse them).
 *   Refused (HIFIHR_EINVAL, nothing launched or written): n / B <= 0, out_size outside 1 .. 256, NULL open_2dj_d / open_2dj_con_d /
 *   packed_d, both outputs NULL.
 *
 * hifihr_ho3d_depth_crop: the metric depth through the same crop box, one thread per output pixel, a plain gather, no workspace.
 *   Cache (device): depth_u16_d[n][FH][FW] uint16, the dataset's encoding decoded (blue + 256 green of the depth PNG:
 *   hifihr_amd.data.ho3d_depth_to_u16); depth_scale = metres per unit (HO-3D: 0.00012498664727900177, :1040).
 *   out_depth_d[B][S][S], S = out_size: out[b][r][q] = (float)u16[idx[b]][sy(r)][sx(q)] * depth_scale, one float32 product, with
 *     sx(q) = x0 + floor((q + 0.5) (x1 - x0) / S),  sy(r) = y0 + floor((r + 0.5) (y1 - y0) / S),  the division and the floor in double,
 *   (x0, y0, x1, y1) the rounded box of packed_d: Pillow's Image.crop(box).resize((S, S), NEAREST) of the 16-bit image.  Exactly 0 where the
 *   source position lies outside the frame, where the stored value is 0 (no measurement), for an index outside 0 .. n - 1 and for a box that
 *   is empty, inverted or longer than HIFIHR_HO3D_MAX_WINDOW on an edge.
 *   A deliberate departure from the reference, which resizes the two byte planes of the encoded image bilinearly and decodes afterwards
 *   (:1169-1171): wrong wherever the low byte wraps and at every depth edge.  A depth image is gathered, never averaged.
 *   Refused (HIFIHR_EINVAL, nothing launched or written): n / B / FH / FW <= 0, out_size outside 1 .. 256, NULL depth_u16_d / packed_d /
 *   out_depth_d. */
int hifihr_ho3d_keypoints(const float* open_2dj_d, const float* open_2dj_con_d, int n, const int* packed_d, int B, int out_size,
                          float* out_open_2dj_d, float* out_con_d, void* stream);
int hifihr_ho3d_depth_crop(const uint16_t* depth_u16_d, int n, int FH, int FW, const int* packed_d, int B, int out_size, float depth_scale,
                           float* out_depth_d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth map to points: a fixed-size point cloud from a depth map, the reference's utils/fh_utils.py:685-717 (batch_depth2pc) as ONE
 * launch, one workgroup per sample; the input of the `chamfer` / `point_mesh` terms (examples["chamfer_points"]).
 *   depths_d[B][H][W] fp32 (0 = no measurement), K_d[B][3][3] the intrinsics of THAT map (its resolution, its axes),
 *   mask_d[B][H][W] float32 (mask_i64 = 0) or int64 (mask_i64 = 1), or NULL; draws_d[B][P] fp32 in [0, 1); origin_d[B][3] or NULL.
 * Valid pixels: (r, q) of sample b is valid when depths[b][r][q] > 0 and, with a mask, mask[b][r][q] != 0.  n_b is their number,
 *   out_count_d[b] = n_b; they are ordered row-major.
 * Draw: k_i = min(n_b - 1, (int)floorf(draws[b][i] * (float)n_b)), the product a float32 multiply (the clamp is needed: 1 - 2^-24 times
 *   2^17 rounds to 2^17; a draw below 0 or not a number takes k = 0).  Uniform, WITH replacement, over ALL valid pixels: a fixed number of
 *   points per sample, no per-sample counts.  The reference's randint(0, n - 1) never draws the last valid pixel; that off-by-one is not
 *   reproduced.
 * Point: the k_i-th valid pixel (r, q) with d = depths[b][r][q] gives out_points_d[b][i] = K_b^-1 . (u d, v d, d) - origin[b],
 *   u = q + c, v = r + c, computed in double and rounded ONCE to float32.  K^-1 is the closed-form adjugate over the determinant of the full
 *   3 x 3 matrix, without contraction; a singular K gives values that are not finite.  d is the PROJECTIVE depth (K p)_z: with a third
 *   row (0, 0, 1) that is z, with HO-3D's raw (0, 0, -1) it is -z.
 *   c = 0.5, the pixel-centre offset of this project's camera: the rasteriser's sample i of an S-wide grid sits at NDC (2 i + 1) / S - 1
 *   (csrc/render_math.h pix_to_ndc), which Model.camera_from_K maps to pixel coordinate i + 0.5; the kernel derives c from pix_to_ndc, and
 *   the closed-loop test (tests/ho3d_extras_cases.py) holds it there.
 *   For an upper-triangular K this is the reference's x = (u - cx) z / fx; what remains different is the reference's +1e-5 on the focal
 *   length, its c = 0 and its float32 arithmetic.
 *   out_index_d[B][P] int32 (may be NULL): the chosen pixel r W + q.
 * n_b = 0: that sample's points are zeros (a target at the origin: check out_count_d), its indices -1.  n_b = 1: P copies of the one point.
 * No atomics, no workspace, no allocation, nothing read back: capturable; the same draws give the same bits on every call.
 * Refused (HIFIHR_EINVAL, nothing launched or written): B / P / H / W <= 0, H W > HIFIHR_DEPTH_POINTS_MAX_PIXELS (the validity words and
 * their prefix counts live in LDS), NULL depths_d / K_d / draws_d / out_points_d / out_count_d.
 * ---------------------------------------------------------------------------------------------- */
#define HIFIHR_DEPTH_POINTS_MAX_PIXELS (512 * 512)
int hifihr_depth_points(const float* depths_d, const float* K_d, const void* mask_d /* or NULL */, int mask_i64,
                        const float* draws_d, const float* origin_d /* or NULL */, int B, int H, int W, int P, float* out_points_d,
                        int32_t* out_count_d, int32_t* out_index_d /* or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIFIHR_H */
