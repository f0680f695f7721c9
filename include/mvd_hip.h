/* mvd_hip.h -- C ABI of libmvd_hip.so: the MI355X (gfx950) implementation of the
 * pananananas/MVD denoising hot path.
 *
 * The reference has no FFI of its own: its boundary is the Python object protocol of
 * MultiViewUNet.forward (/root/reference/src/models/mvd_unet.py:179-191) which calls
 * diffusers' UNet2DConditionModel (mvd_unet.py:318-326, image_encoder.py:105-110),
 * ImageCrossAttentionProcessor.__call__ (attention.py:48-188) and
 * CameraEncoder.{encode_cameras,apply_modulation} (camera_encoder.py:160-255).
 * This header is what a binding for that path binds instead (ctypes stub: INTEGRATION.md).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _host;
 *  - no torch / C++ types; sizes are explicit; the caller owns every buffer;
 *  - work is issued asynchronously on the hipStream_t passed as `void* stream`;
 *  - every function returns 0 on success, <0 on error; mvd_last_error() returns the
 *    message of the calling thread's last failure;
 *  - one calling thread per engine handle.
 */
#ifndef MVD_HIP_H
#define MVD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVD_MAX_LEVELS 4

/* UNet2DConditionModel config subset (diffusers 0.32.2 names; SD-2.1 values in comments).
 * Replaces: UNet2DConditionModel.from_pretrained(...).config  (mvd_unet.py:46-53). */
typedef struct {
  int in_channels;                         /* 4 */
  int out_channels;                        /* 4 */
  int num_levels;                          /* 4 */
  int block_out_channels[MVD_MAX_LEVELS];  /* 320 640 1280 1280 */
  int num_heads[MVD_MAX_LEVELS];           /* 5 10 20 20 ("attention_head_dim") */
  int layers_per_block;                    /* 2 */
  int cross_attention_dim;                 /* 1024 */
  int norm_num_groups;                     /* 32 */
  float norm_eps;                          /* 1e-5 */
  /* MVD wrapper (mvd_unet.py:23-36) */
  int cam_output_dim;                      /* 1024 */
  int cam_hidden_dim;                      /* 512 */
  int simple_cam_encoder;                  /* 0 */
  float cam_modulation_strength;           /* 0.2 */
} mvd_config_t;

typedef struct mvd_engine mvd_engine_t;

const char* mvd_last_error(void);

/* ---- engine lifetime -------------------------------------------------------------- */
int mvd_engine_create(const mvd_config_t* cfg, mvd_engine_t** out);
int mvd_engine_destroy(mvd_engine_t* e);

/* Packed-weight registration.  `set` 0 = base_unet (+ adapter processors + camera encoder),
 * 1 = image_encoder.unet.  Slot names and layouts: DESIGN.md "Weight slots".
 * dtype: 0 = fp32, 1 = bf16.  The engine keeps the pointer; the caller keeps the memory alive.
 * Replaces: nn.Module.load_state_dict / .to(device) of mvd_unet.py:164-177, infer.py:67-76. */
int mvd_engine_set_weight(mvd_engine_t* e, int set, const char* slot, const void* ptr, int64_t numel, int dtype);
int mvd_engine_clear_weights(mvd_engine_t* e, int set);

/* Workspace: bytes needed for one forward at the given shape (dry run of the schedule). */
int64_t mvd_engine_workspace_bytes(mvd_engine_t* e, int batch, int height, int width, int text_len, int ref_batch);
/* Persistent bytes for the cached reference K/V (and kept feature maps when keep_features). */
int64_t mvd_engine_refcache_bytes(mvd_engine_t* e, int ref_batch, int height, int width, int keep_features);
int mvd_engine_bind_workspace(mvd_engine_t* e, void* ws, int64_t ws_bytes, void* refcache, int64_t refcache_bytes);

/* ---- the hot path ------------------------------------------------------------------ */
enum {
  MVD_USE_CAMERA = 1,       /* use_camera_conditioning and target_camera is not None (mvd_unet.py:241) */
  MVD_USE_IMAGE = 2,        /* use_image_conditioning and source_image_latents is not None (:269)      */
  MVD_REUSE_REF = 4,        /* reuse reference K/V computed by a previous call (inputs step-invariant)  */
  MVD_KEEP_FEATURES = 8,    /* keep the 16 encoder feature maps for mvd_engine_get_feature               */
  MVD_SHARE_REF = 16,       /* `views` views of ONE object in one forward, sharing one reference (below)  */
  MVD_DEEPCACHE_REFRESH = 32, /* the ordinary forward, which also stores the deep feature (DeepCache, below)  */
  MVD_DEEPCACHE_SHALLOW = 64  /* the shallow forward: the stored deep feature in place of the deep layers       */
};

/* The batch layout of a forward, described once for the three entries below (the engine holds it as one value, csrc/ragged.h):
 * O objects, object o seen from V_o views, R = sum of the V_o, g rows per view (1, or 2 under classifier-free guidance).  The
 * sample holds g * R rows [uncond x R | cond x R], object-major inside a half: row r = j * R + c, c = (views of the objects before
 * o) + v, is row j of the batch-g call of view v of object o with a one-row reference.  It attends tokens [j * hw / g,
 * (j + 1) * hw / g) of object o's reference and text row j * O + o, takes camera c (or the one camera) and timesteps[r];
 * `source_latents` / `encoder_text` hold O rows, `text` g * O, the cameras 0, 1 or R; hw % g == 0 at every level; all of it is
 * checked on the host before any launch, in the words of the entry that was called.  The forms: one object and V views --
 * MVD_SHARE_REF with args->views = V on mvd_unet_forward; O objects x V views -- the object count beside the block,
 * mvd_unet_forward_objects; counts that differ -- the counts beside the block, mvd_unet_forward_ragged, where equal counts are the
 * objects form and one object the views form, rejections included.  A reference cached under one layout is never served to another.
 *
 * MVD_SHARE_REF (with MVD_USE_IMAGE; no counterpart in the reference, whose infer.py:111-122 makes one batch-1 call per
 * view): the forward computes what `views` independent forwards of batch g = batch / views (1, or 2 under classifier-free
 * guidance) with a ONE-row reference compute, from one encoder pass and one copy of the reference K/V: the layout above with
 * O = 1, R = views (Q4 at batch g in both adapter branches; camera v by the existing r % cam_batch rule).  The encoder pass, the
 * Q2 statistics and the ref_kv projection run once, at ref_batch = 1.  The flag is rejected on mvd_engine_reference_encode too (the global-statistics path is for batches
 * sharded over ranks: more than one object).  Size the workspace with mvd_engine_workspace_bytes_args. */

/* One MultiViewUNet.forward (mvd_unet.py:179-338).  All tensors fp32, contiguous. */
typedef struct {
  int batch;                 /* rows of `sample` (2B under classifier-free guidance)                    */
  int height, width;         /* latent spatial size (64x64 for 512x512 images)                           */
  int text_len;              /* 77                                                                       */
  const float* sample;       /* [batch][in_channels][H][W]                                               */
  const float* timesteps;    /* [batch] (already expanded; ints as floats)                               */
  const float* text;         /* [batch][text_len][cross_attention_dim] (already repeated, :233-237);
                                MVD_SHARE_REF: [batch / views] rows (one per guidance half)               */
  const float* source_camera;/* [batch][cam_rows][4] or NULL                                             */
  const float* target_camera;
  int cam_rows;              /* 3 or 4 (Q8)                                                              */
  int cam_batch;             /* rows of the camera tensors: 0 or `batch`, or a divisor of `batch` (1 = torch's
                                (1,C,1,1) broadcast; under CFG the 2B latents share the B cameras: row b uses
                                camera b % cam_batch) -- pipeline.py:141-152                                   */
  const float* fourier_proj; /* [cam_output_dim][6*((cam_output_dim/2)/3)] the per-call random matrix Q1 */
  const float* source_latents;/* [ref_batch][in_channels][H][W] or NULL                                  */
  const float* encoder_text; /* [ref_batch][text_len][xdim]: text rows chosen per mvd_unet.py:278-285     */
  int ref_batch;
  int flags;
  float* out;                /* [batch][out_channels][H][W]                                              */
  int views;                 /* MVD_SHARE_REF: views per object (>= 1, divides batch); otherwise 0 or 1   */
} mvd_forward_args_t;

int mvd_unet_forward(mvd_engine_t* e, const mvd_forward_args_t* args, void* stream);
/* mvd_engine_workspace_bytes for a whole argument block (shapes, flags, ref_batch, cam_batch, views; the pointers are not
 * read): the only sizing entry for an MVD_SHARE_REF forward, which the positional form cannot describe. */
int64_t mvd_engine_workspace_bytes_args(mvd_engine_t* e, const mvd_forward_args_t* args);

/* Several objects in one MVD_SHARE_REF forward (turntables of a list of objects; mvd_forward_args_t is unchanged, the object
 * count comes beside it).  A forward of O objects x V = args->views views with g rows per view (1, or 2 under guidance) IS the
 * O * V independent forwards of batch g, each with a one-row reference.  The sample holds g * O * V rows in the pipeline's
 * order [uncond x O V | cond x O V], object-major inside a half; row r = j * O * V + o * V + v
 *   - attends, in both adapter branches and all 16 features, tokens [j * hw / g, (j + 1) * hw / g) of object o's reference only
 *     (the reference K/V hold O * g elements of hw / g rows, object-major: element o * g + j);
 *   - attends text row j * O + o (`text` holds g * O rows, [negative x O | positive x O]);
 *   - takes camera o * V + v (cam_batch = O * V, or 1) and timesteps[r].
 * The encoder pass runs once at batch O (`source_latents`, `encoder_text`: O rows, row o what object o's own call would use), the
 * Q2 statistics are taken per object (per pixel over that object's channels only: mvd_op_refnorm at batch 1), the ref_kv
 * projection runs once over O * hw rows and the reference cache is that of ref_batch = O.  Every object has the same V.
 * Shapes and checks: the layout above with R = O * views.  objects <= 1: exactly mvd_unet_forward /
 * mvd_engine_workspace_bytes_args, with their rejections. */
int mvd_unet_forward_objects(mvd_engine_t* e, const mvd_forward_args_t* args, int objects, void* stream);
int64_t mvd_engine_workspace_bytes_objects(mvd_engine_t* e, const mvd_forward_args_t* args, int objects);

/* Ragged turntables: O objects with view_counts[o] >= 1 views each in one MVD_SHARE_REF forward (mvd_forward_args_t is unchanged
 * and args->views must be 0: the counts come beside it).  With R = sum of the counts and g rows per view (1, or 2 under
 * guidance) the forward IS the R independent forwards of batch g, each with a one-row reference -- the definition of
 * mvd_unet_forward_objects with V per object, and the layout above as it stands (row r reads K/V element o * g + j of the O * g
 * the ref_kv projection writes object-major).
 * Encoder pass, Q2 statistics, ref_kv projection and reference cache are those of mvd_unet_forward_objects at ref_batch = O.
 * The two row maps are tables the engine builds from the counts (valid by construction, and checked on the host like any
 * table: 0 <= entry < g * O) and keeps in device slots keyed by (counts, g).  A slot is written once, by a stream-ordered
 * upload on the first forward of its layout, which therefore cannot run inside a stream capture of the caller's; no later
 * forward of that layout uploads or synchronises.  At most 8 layouts are resident: a ninth evicts the least recently used
 * one after dropping every captured hipGraph of the engine (mvd_engine_set_graph), so a slot a live graph points at is
 * never rewritten.
 * Shapes and checks: the layout above, and before it args->views == 0, every count >= 1 and batch == g * R.  Equal counts run
 * mvd_unet_forward_objects (one object: the `views` forward) -- the same code, bit-identical results, their rejections.
 * The reference-cache record and the hipGraph key carry the counts. */
int mvd_unet_forward_ragged(mvd_engine_t* e, const mvd_forward_args_t* args, const int* view_counts, int objects, void* stream);
int64_t mvd_engine_workspace_bytes_ragged(mvd_engine_t* e, const mvd_forward_args_t* args, const int* view_counts, int objects);

/* Global Q2 statistics (SURVEY.md 8e mode ii; optional).  The adapter normalises the reference features with statistics
 * over (batch, channel) per pixel (attention.py:95-103), so a batch sharded over GPUs sees per-shard statistics unless the
 * shards exchange them.  The reference pass is therefore also available in two halves:
 *   mvd_engine_reference_encode   runs the image-encoder pass for `args` (uses height, width, text_len, ref_batch,
 *                                 source_latents, encoder_text), keeps the 16 raw feature maps in the reference cache (bind it
 *                                 with keep_features = 1) and writes the LOCAL per-pixel pair (mean, M2 = sum of squared
 *                                 deviations from that mean) over ref_batch x C of every feature to
 *                                 local_stats[mvd_engine_reference_pixels()][2], features concatenated in encoder order;
 *   (the host merges the ranks' pairs -- one all-gather of 215 KB at 64x64 -- into mean and k = 0.5 / max(std, 1e-6))
 *   mvd_engine_reference_finish   normalises with mean_k[pixels][2] = (mean, k) and projects to the adapter K/V.
 * Afterwards mvd_unet_forward with MVD_USE_IMAGE | MVD_REUSE_REF runs the main pass on that reference.  With one rank the
 * three calls reproduce the ordinary forward.  There is no counterpart in the reference (its DDP replicas normalise
 * locally); mvd_amd.distributed.merge_reference_stats is the host side. */
int64_t mvd_engine_reference_pixels(mvd_engine_t* e, int height, int width);
int mvd_engine_reference_encode(mvd_engine_t* e, const mvd_forward_args_t* args, float* local_stats, void* stream);
int mvd_engine_reference_finish(mvd_engine_t* e, const float* mean_k, void* stream);

/* hipGraph replay of whole forwards.  When enabled, a mvd_unet_forward whose argument block (every pointer, shape and flag),
 * bound buffers and starting reference-cache state were seen before is replayed as ONE hipGraphLaunch: the first call with
 * such a key runs normally, the second is stream-captured and instantiated, later ones replay (up to 8 graphs are kept;
 * registering weights, re-binding buffers or disabling the switch drops them).  The caller must therefore pass the SAME
 * device buffers every step and refresh their contents in place, on a non-default stream (a capture on the legacy stream is
 * illegal).  Ignored while profiling is on.  Mirrors SURVEY.md section 7 step 7; there is nothing like it in the reference. */
int mvd_engine_set_graph(mvd_engine_t* e, int enable);

/* N4 (training.py:60-65, config/train_config.yaml:43): when the image encoder's UNet weights are identical to the
 * base UNet's (frozen base), the encoder pass can read weight set 0 and set 1 need not be registered at all. */
int mvd_engine_share_encoder_weights(mvd_engine_t* e, int enable);

/* Main-pass options: what setting or clearing one invalidates.  FreeU, token merging, token downsampling, DeepCache and the taps
 * (below) are state of the engine, beside the argument block; every forward entry honours them and the workspace entries size the
 * forward of the CURRENT setting.  Every setter and clearer drops the captured hipGraphs, and besides:
 *   set_freeu / clear_freeu                           nothing more
 *   set_tome / clear_tome                             the kept slot tables
 *   set_todo / clear_todo                             the key counts, DeepCache's stored feature
 *   set_deepcache / clear_deepcache / bind_deepcache  DeepCache's stored feature
 *   set_taps                                          the tap records
 * (FreeU and token merging leave a stored deep feature valid.)  A refused call (-1 and a message) changes nothing.
 *
 * FreeU (Si et al., CVPR 2024; diffusers-0.32.2 UNet2DConditionModel.enable_freeu(s1, s2, b1, b2), restated) on the MAIN UNet
 * pass: in front of every resnet of up block 0 (b1, s1) and of up block 1 (b2, s2) the hidden input and the skip input are
 * replaced by mvd_op_freeu's two outputs (below); up blocks 2 and 3 are untouched.  The encoder pass, the Q2 statistics, the
 * reference K/V and the reference cache never depend on the setting (also with mvd_engine_share_encoder_weights).  A workspace
 * bound before FreeU was set may be too small: the forward then says so before it launches anything.  All four values must be
 * positive and finite, else -1.  Clear (the default): the launches of a forward are what they were. */
int mvd_engine_set_freeu(mvd_engine_t* e, float s1, float s2, float b1, float b2);
int mvd_engine_clear_freeu(mvd_engine_t* e);

/* Token merging (mvd_op_tome_* below) in front of attn1 of the MAIN pass's transformer blocks whose map
 * H x W of a latent H0 x W0 has ceil(sqrt((H0 W0) / (H W))) <= max_downsample, with r = min(ns, int(H W ratio)) > 0: LayerNorm1,
 * match + select, merge, the plain attn1.qkv GEMM on B N' rows, the one- or two-problem attention with nq = nk_self = N' (the
 * adapter's Q_ref from merged rows, the reference K/V at full length), the out-projection into a temporary, un-merge + add.  attn2
 * and the feed-forward are as they were; the encoder pass and the reference K/V never merge.  ratio in [0, 0.75], max_downsample
 * one of 1, 2, 4, 8, else -1.  ratio 0, or no eligible block: the launches of a forward are what they were.  A merging block
 * whose map is above the select kernel's limit or whose channels are no multiple of 64 fails the forward before anything is
 * launched.  What setting or clearing invalidates: "main-pass options" above.
 * keep_tables (test plumbing): every merging block's slot table [batch][H W] stays in the workspace after the forward;
 * mvd_engine_tome_table copies that of feature `feature_idx` of the last issued forward to the device array `out` and returns
 * its length (0: the block did not merge; out null: the length alone). */
int mvd_engine_set_tome(mvd_engine_t* e, double ratio, int max_downsample, int keep_tables);
int mvd_engine_clear_tome(mvd_engine_t* e);
int64_t mvd_engine_tome_table(mvd_engine_t* e, int feature_idx, int* out, void* stream);

/* Token downsampling (ToDo: Smith, Saxena and Saha, IJCAI 2024, restated; mvd_op_todo_downsample below)
 * of the keys and values of attn1 in the MAIN pass's transformer blocks.  A block whose map is H x W of a latent H0 x W0 has
 * down = ceil(sqrt((H0 W0) / (H W))) (token merging's rule); down 1 takes `factor`, down 2 `factor_level_2`, a deeper block is never
 * downsampled.  With a factor f in {2, 3, 4} and H / f >= 1, W / f >= 1 the block runs the fused LayerNorm + q/k/v GEMM as ever, ONE
 * pooling launch of the K and V columns into a compact [batch][Nk][2C] buffer, Nk = (H / f)(W / f), and the attention launch with
 * nq = H W queries against nk = Nk keys; the adapter's self branch (Q_ref of all H W rows against the reference K/V at full
 * length, every layout map), the out-projection with the residual, attn2, the feed-forward, the encoder pass and the cached
 * reference are what they were.  method 0: nearest (the top-left token of each cell), 1: area (the cell's mean).
 * A factor outside [1, 4] or a method outside {0, 1}: -1.  While token merging is set (ratio > 0) set_todo with a factor above 1 is
 * refused, and mvd_engine_set_tome with a ratio above 0 is refused while a factor is above 1: -1 and a message, nothing changes.
 * Both factors 1, or clear: the launches of a forward are what they were.  What setting or clearing invalidates: "main-pass
 * options" above (a deep feature of another setting is stale).  mvd_engine_todo_keys: out[i], i < min(n, features) = Nk of feature
 * i's block in the last issued forward (0: it was not downsampled, or no forward yet); host memory; returns the number of features. */
int mvd_engine_set_todo(mvd_engine_t* e, int factor, int factor_level_2, int method);
int mvd_engine_clear_todo(mvd_engine_t* e);
int mvd_engine_todo_keys(mvd_engine_t* e, int* out, int n);

/* DeepCache (Ma et al., CVPR 2024; the DeepCacheSDHelper used with diffusers, restated): the deep, low-resolution features of
 * the main pass change little between neighbouring denoising steps, so a step may reuse them.  With n = num_levels,
 * Lb = layers_per_block, a branch b in [0, Lb) (DeepCache's cache_branch_id) and j0 = Lb - 1 - b, the DEEP FEATURE is the hidden
 * (not the skip) input of up_blocks.{n-1}.resnets.{j0} in the main pass: for j0 >= 1 the output of up_blocks.{n-1}.attentions.{j0-1},
 * for j0 = 0 the up-sampled output of up block n-2 after its FiLM hook; [batch][H][W][C] bf16, C = block_out_channels[0] (j0 >= 1) or
 * block_out_channels[1] (j0 = 0).
 *   MVD_DEEPCACHE_REFRESH  the ordinary forward (every flag and layout as without the bit, the same output bit for bit), which also
 *                          copies the deep feature into the bound buffer (one device-to-device copy on the forward's stream).
 *   MVD_DEEPCACHE_SHALLOW  the front matter (time, camera and text paths, im2col with the input FiLM), the text K/V GEMM, conv_in,
 *                          down_blocks.0 layers 0..b (resnet + transformer each; no downsampler, no down_0 hook), then
 *                          up_blocks.{n-1} layers j0..Lb starting from the STORED feature (layer j reads the skip of down layer
 *                          Lb - j, conv_in's output for j = Lb), the up_{n-1} hook, conv_norm_out, conv_out.  Nothing else runs: it is
 *                          the full forward with that one tensor replaced by the stored one.  Every executed layer reads the time
 *                          projection, text K/V, reference K/V and per-row K/V maps of its position in the FULL schedule.  With
 *                          MVD_USE_IMAGE it needs MVD_REUSE_REF and a matching cached reference: the encoder pass never runs and
 *                          the side stream is never forked.  FreeU applies to the executed resnets it applies to in a full forward.
 * Both bits together, either bit without mvd_engine_set_deepcache, or on mvd_engine_reference_encode: -1, nothing is launched.
 * The stored feature carries a record -- batch, height, width, the batch layout, the MVD_USE_CAMERA / MVD_USE_IMAGE bits, the
 * branch and a weight generation that mvd_engine_set_weight / mvd_engine_clear_weights bump -- and a shallow forward whose
 * arguments do not match it is rejected before any launch, in words that name the mismatch.  The timestep is not part of the
 * record: reusing the feature at another step is the point.  The bits are part of the argument block and so of the hipGraph key.
 *   mvd_engine_set_deepcache / _clear_deepcache   set the branch (outside [0, Lb): -1) / switch off
 *   mvd_engine_deepcache_bytes / _bind_deepcache  the buffer of the stored feature for a forward of this shape (any branch), apart
 *                          from the reference cache (whose allocator every cold forward resets); 256-byte aligned.
 * What setting, clearing or binding invalidates: "main-pass options" above.
 * The mvd_engine_workspace_bytes_args / _objects / _ragged entries size the forward the bits describe; a shallow forward never
 * needs more than the full forward of the same arguments (checked there). */
int mvd_engine_set_deepcache(mvd_engine_t* e, int branch);
int mvd_engine_clear_deepcache(mvd_engine_t* e);
int64_t mvd_engine_deepcache_bytes(mvd_engine_t* e, int batch, int height, int width);
int mvd_engine_bind_deepcache(mvd_engine_t* e, void* ptr, int64_t bytes);

/* Per-kernel-class timing with HIP events on the launch stream (measurement only; off by default).
 * classes = kernels: 0..5, 12 lock-step GEMM/conv tile configs (gemm.hip); ping-pong 256x320 kernels (gemm_pp.hip): 7 dense,
 * 13 implicit-GEMM 3x3 convolution, 14 split-K, 6 GEGLU; 8..11 attention (1,2,4,8 waves); 16 groupnorm; 17 layernorm. */
int mvd_engine_set_profiling(mvd_engine_t* e, int enable);
int mvd_engine_profile_summary(mvd_engine_t* e, int cap, int* cls, int* launches, double* ms, double* flops, double* bytes);
/* Per-shape text table ("cls M N K tag launches ms tflops" per line) of the launches recorded since profiling was
 * enabled, written to a HOST buffer; call before mvd_engine_profile_summary (which resets the records).
 * Returns the number of bytes written (<0 on error). */
int mvd_engine_profile_shapes(mvd_engine_t* e, char* buf_host, int cap);

/* Main-pass taps (test plumbing, off by default).  With taps on, a forward records every block output of its MAIN pass, in
 * execution order, under these names:
 *   conv_in; down_blocks.i.resnets.j, down_blocks.i.attentions.j, down_blocks.i.downsamplers.0; mid_block.resnets.0,
 *   mid_block.attentions.0, mid_block.resnets.1; up_blocks.i.resnets.j, up_blocks.i.attentions.j, up_blocks.i.upsamplers.0;
 *   film.down_i / film.up_i, the output of each FiLM hook (MVD_USE_CAMERA; "mid_0" is the identity and has none);
 *   conv_norm_out.in, the hidden state that enters conv_norm_out (the tensor of the last tap before it).
 * A DeepCache shallow forward records the blocks it executes.  The encoder pass has no taps (mvd_engine_get_feature reads its
 * outputs).  The tapped tensors are the pass's own activations, which stay in the workspace until the next call that uses it;
 * the FiLM hooks of the mid and up blocks, which otherwise modulate in place, write a tensor of their own while taps are on
 * (the same launch; the block output in front of the hook stays readable), and the mvd_engine_workspace_bytes* entries count
 * it.  No launch and no synchronisation is added, the forward's output is bit for bit what it is with taps off, and with taps
 * off a forward and its workspace size are what they were.  What mvd_engine_set_taps invalidates: "main-pass options" above
 * (a graph's FiLM hooks write where they wrote when it was captured); a replayed graph restores the records of the forward it captured.
 *   mvd_engine_num_taps   the number of records of the last issued forward (-1 with taps off)
 *   mvd_engine_tap_info   name (a host buffer of `cap` bytes) and shape of record `idx`
 *   mvd_engine_get_tap    the tensor [batch][height][width][channels] bf16 as out_nchw [batch][channels][height][width] fp32 */
int mvd_engine_set_taps(mvd_engine_t* e, int enable);
int mvd_engine_num_taps(mvd_engine_t* e);
int mvd_engine_tap_info(mvd_engine_t* e, int idx, char* name, int cap, int* batch, int* channels, int* height, int* width);
int mvd_engine_get_tap(mvd_engine_t* e, int idx, float* out_nchw, void* stream);

/* Number / shape / copy-out (NCHW fp32) of the encoder feature maps (image_encoder.py:36-84). */
int mvd_engine_num_features(mvd_engine_t* e);
int mvd_engine_feature_shape(mvd_engine_t* e, int idx, int* channels, int* height, int* width);
int mvd_engine_get_feature(mvd_engine_t* e, int idx, float* out_nchw, void* stream);
/* CameraEncoder.encode_cameras (camera_encoder.py:160-176): cameras [batch][cam_rows][4] -> out_emb [batch][cam_output_dim] */
int mvd_engine_encode_cameras(mvd_engine_t* e, const float* source_camera, const float* target_camera, int cam_rows,
                              int batch, const float* fourier_proj, float* out_emb, void* stream);
/* CameraEncoder.apply_modulation_to_tensor (camera_encoder.py:207-255) on x [batch][channels][hw] fp32.
 * Returns 1 (and writes nothing) when `name` is not a modulator -- the reference's silent identity (Q3). */
int mvd_engine_apply_modulation(mvd_engine_t* e, const char* name, const float* emb, int batch, const float* x_nchw,
                                int channels, int hw, float* out_nchw, void* stream);
/* Camera embedding of the last forward ([batch][cam_output_dim] fp32), for parity tests. */
int mvd_engine_get_camera_embedding(mvd_engine_t* e, float* out, void* stream);
/* FiLM parameters of every hooked modulator (down_i, up_i, output: the forward's order) from an embedding emb [cam_batch][
 * cam_output_dim], through the function the forward's camera path runs (the concatenated form when the cam.modcat.* slots are
 * registered, else one modulator at a time).  out, in the engine's own layout: per modulator scale [out_rows][dim] | shift
 * [out_rows][dim]; rows beyond cam_batch repeat the cameras cyclically (row r = camera r % cam_batch). */
int mvd_engine_film_params(mvd_engine_t* e, const float* emb, int cam_batch, int out_rows, float* out, void* stream);
/* The forward's time path on weight set 0: timesteps [batch] -> out [batch][sum of resnet cout] fp32, every resnet's
 * time_emb_proj output (bias included) in module order. */
int mvd_engine_time_projection(mvd_engine_t* e, const float* timesteps, int batch, float* out, void* stream);

/* ---- operator-level entry points (same kernels the engine schedules; used by tests) -- */
/* out[M][N] = alpha*(A[M][K] . W[N][K]^T + bias + rowvec[m/rows_per_batch]) + res ; bf16 A/W/res
 * Rounding contract: the sum and the whole epilogue are fp32 and the result is rounded ONCE, to nearest even, when it is stored
 * as bf16 (out_f32: not at all) -- in every tile config, the split-K forms (separate reduce and in-kernel combine), the small-M
 * kernels with either weight layout, the X-stationary form and the convolutions below; no form adds res, bias or rowvec behind
 * a rounding.  tests/test_exact_gemm_gpu.py and tests/test_exact_conv_gpu.py compare bitwise against exactly this order. */
int mvd_op_linear(const void* a, const void* a2, int k1, int k2, const void* w, const float* bias, const float* rowvec,
                  int ld_rowvec, int rows_per_batch, const void* res, float alpha, int geglu, void* out, int out_f32,
                  int m, int n, int force_cfg, int splitk, float* splitk_ws /* splitk*m*n floats when splitk > 1 */,
                  void* stream);
/* mvd_op_linear with the leading dimensions of the engine's own call sites: W is [n][ldw] with ldw >= k1 + k2 (only the first
 * k1 + k2 elements of a row are read, only the first n rows), res is [m][ldres] and out [m][ldo] -- column slices of wider
 * buffers; res == out runs in place.  ldw % 8 == 0, ldres % 4 == 0, ldo % 4 == 0; the row vector's base is 16-byte aligned
 * and ld_rowvec % 4 == 0.  A stride some kernel family cannot take is an error, or another kernel of the same tile, never a
 * misaligned access: the ping-pong kernels (config 6 / 7) need ldo % 8 == 0 and ldres % 8 == 0 and leave other strides to the
 * lock-step 256x320 tile; the blocked weight layout (force_cfg + 1000) has no row stride: ldw == k1 + k2.
 * tests/test_exact_strides_gpu.py compares these forms bitwise. */
int mvd_op_linear_ld(const void* a, const void* a2, int k1, int k2, const void* w, int ldw, const float* bias, const float* rowvec,
                     int ld_rowvec, int rows_per_batch, const void* res, int ldres, float alpha, int geglu, void* out, int ldo,
                     int out_f32, int m, int n, int force_cfg, int splitk, float* splitk_ws /* splitk*m*n floats when splitk > 1 */,
                     void* stream);
/* out[M][N] = LayerNorm(x[M][K]; gamma, beta, eps) . W^T + b in ONE kernel (geglu = 1: followed by value*gelu(gate), width
 * N/2, rows interleaved as for mvd_op_linear).  w_folded = W.diag(gamma) in bf16, c1[n] = sum_k w_folded[n][k] (of the bf16
 * values, fp32), c2[n] = sum_k beta[k].W[n][k] + b[n]: mvd_amd/packing.py::fold_layernorm.  Shapes: K <= 1280, N % 320 == 0
 * and enough rows for the 256x320 tile grid (M*N >= 200 tiles); anything else returns an error (the engine then runs the
 * LayerNorm kernel + mvd_op_linear). */
int mvd_op_ln_linear(const void* x, int k, const void* w_folded, const float* c1, const float* c2, float eps, int geglu,
                     void* out, int m, int n, void* stream);
/* The X-stationary short-K form (mvd_amd/csrc/gemm_xs.hip; K = 320, the 64x64 level of SD-2.1 at many rows):
 *   out[M][units*32] = LN?(x[M][K]) . W^T + b (+ res)        geglu = 1: out[M][units*16] = value * gelu_erf(gate)
 * x rows stay in registers, w_packed is the fragment-ordered weight stream of mvd_amd/packing.py::pack_xs (bias included;
 * ln = 1: packed from the LayerNorm-folded pair of fold_layernorm).  csplit <= 0: heuristic column split.
 * Replaces, for those shapes, the Linear / GEGLU projections of diffusers' BasicTransformerBlock that
 * /root/reference/src/models/mvd_unet.py:318-326 reaches through UNet2DConditionModel.forward. */
int mvd_op_linear_xs(const void* x, int ldx, const void* w_packed, int m, int k, int units, int geglu, int ln, float ln_eps,
                     const void* res, int ldres, void* out, int ldo, int csplit, void* stream);
/* The weight-streaming form of a resnet 3x3 convolution on ONE image's small map (mvd_amd/csrc/conv_ws.hip: batch 1, the 8x8 and
 * 16x16 levels -- 15-65 MB of weights for a few GFLOP):  out[B*H*W][n] = conv3x3(x; stride 1, pad 1) (+ [sc | sc2] . Wsc^T) + bias
 * + rowvec[image] + res.  w in {8, 16, 32}, h*w % 64 == 0, B*h*w <= 1024, c % 128 == 0, sc_c1 / sc_c2 % 128 == 0, n % 16 == 0;
 * w_packed from mvd_amd/packing.py::pack_ws; variant 0 = the launcher's choice of block height (1: 64 pixels, 2: 128 pixels on a 16-wide map);
 * + 16: nearest-neighbour 2x upsampling in front of the convolution (diffusers' Upsample2D: output 2h x 2w, 16 or 32 wide, no shortcut).
 * No workspace, no split-K: each workgroup streams its 16-channel weight panel once.
 * Replaces, for those shapes, the Conv2d of diffusers' ResnetBlock2D that /root/reference/src/models/mvd_unet.py:318-326 reaches
 * through UNet2DConditionModel.forward (the reference's own batch-1 loop: /root/reference/infer.py:111-122). */
int mvd_op_conv3x3_ws(const void* x, int batch, int h, int w, int c, const void* w_packed, const float* bias, const float* rowvec,
                      int ld_rowvec, const void* res, const void* sc, const void* sc2, int sc_c1, int sc_c2, void* out, int n,
                      int variant, void* stream);
/* 3x3 conv (pad 1) on NHWC bf16 as implicit GEMM; optional fused 1x1 shortcut on (sc, sc2).  asym_pad = 1 (stride 2 only):
 * zero padding on the bottom/right edge only -- diffusers' VAE Downsample2D(padding=0). */
int mvd_op_conv3x3(const void* x, int batch, int in_h, int in_w, int cin, int stride, int upsample, int asym_pad, const void* w,
                   const float* bias, const float* rowvec, int ld_rowvec, const void* res, const void* sc, const void* sc2,
                   int sc_c1, int sc_c2, void* out, int cout, int force_cfg, int splitk, float* splitk_ws, void* stream);
/* The 3x3 conv behind a nearest-2x upsample (mvd_op_conv3x3 with upsample = 1) as four 2x2 sub-pixel convolutions of the
 * source map: K = 4 * cin instead of 9 * cin.  w4 = mvd_amd.packing.pack_up4: [4 parities][cout][4 * cin] bf16.  256x320
 * ping-pong tile only (force_cfg -1 or 7); cin % 64 == 0, cout % 320 == 0, source width a multiple of 16, or 8 with an even
 * height -- anything else is an error, never another kernel.  out: (batch, 2 in_h, 2 in_w, cout) bf16. */
int mvd_op_conv3x3_up4(const void* x, int batch, int in_h, int in_w, int cin, const void* w4, const float* bias, void* out, int cout,
                       int force_cfg, void* stream);
/* softmax(scale * q.k^T).v per head of 64 channels.  scale == 0 selects the engine's form: q is already multiplied
 * by softmax_scale * log2(e) (the packed to_q / to_q_ref weight rows carry that factor, DESIGN.md "Weight slots"). */
int mvd_op_attention(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq,
                     int ldk, int ldv, int ldo, float scale, void* stream);
/* Grouped K/V: batch element b attends the K/V of K/V batch element b / kv_group, so k / v hold batch / kv_group elements of
 * nk rows (kv_group views of one object share its reference tokens; kv_group <= 1 is mvd_op_attention).  Every wave-count form
 * takes it; bit-identical to running the views one by one. */
int mvd_op_attention_grouped(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq,
                             int ldk, int ldv, int ldo, float scale, int kv_group, void* stream);
/* Grouped K/V of several objects: the batch is [half j][object o][view v] (batch = g * kv_objects * kv_group) over K/V stored
 * object-major, kv_objects * g elements [object o][half j]; with q = b / kv_group, element b attends K/V element
 * (q % kv_objects) * g + q / kv_objects.  kv_objects <= 1 is mvd_op_attention_grouped; kv_group * kv_objects must divide batch. */
int mvd_op_attention_objects(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq,
                             int ldk, int ldv, int ldo, float scale, int kv_group, int kv_objects, void* stream);
/* K/V by table: batch element b attends K/V element kv_index_host[b] of the kv_elements elements k / v hold (ragged view counts
 * per object, any many-to-one map).  kv_index_host is a HOST array of `batch` entries; every entry is checked on the host
 * (0 <= entry < kv_elements) before anything is uploaded or launched, then the table is copied stream-ordered to a
 * library-owned device buffer in front of the launch.  The identity table is mvd_op_attention, the table of
 * mvd_op_attention_objects' map is that entry, bit for bit. */
int mvd_op_attention_mapped(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq,
                            int ldk, int ldv, int ldo, float scale, const int* kv_index_host, int kv_elements, void* stream);
/* Split-KV form (batch 1: too few (head, query block) pairs to fill the chip): the keys are cut into nsplit <= 8 ranges, one
 * workgroup each, merged in the kernel by the last workgroup to arrive.  Prescaled queries only (the scale == 0 form). */
int64_t mvd_op_attention_split_ws_bytes(int batch, int heads, int nq, int nsplit);
int mvd_op_attention_split(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk, int ldq,
                           int ldk, int ldv, int ldo, int nsplit, void* ws, void* stream);
int mvd_op_groupnorm(const void* x0, const void* x1, int c0, int c1, int batch, int hw, int groups, float eps,
                     const float* gamma, const float* beta, int silu, void* y, float* ws, void* stream);
int mvd_op_layernorm(const void* x, int rows, int c, float eps, const float* gamma, const float* beta, void* y,
                     void* stream);
int mvd_op_refnorm(const void* x, int batch, int hw, int c, void* y, void* stream);
/* mvd_op_refnorm with statistics over each run of `group` consecutive batch rows (group divides batch); group == batch is
 * mvd_op_refnorm, group == 1 per object -- bit-identical to mvd_op_refnorm on those rows alone. */
int mvd_op_refnorm_grouped(const void* x, int batch, int group, int hw, int c, void* y, void* stream);
int mvd_op_film(const void* x, int batch, int hw, int c, const float* scale, const float* shift, void* y, void* stream);
int mvd_op_conv_in(const void* x, int batch, int h, int w, int cin, const float* wt, const float* bias, int cout, void* y,
                   void* stream);
int mvd_op_conv_out(const void* x, int batch, int h, int w, int c, const void* wt, const float* bias, int cout, float* y,
                    void* stream);
int mvd_op_nchw_to_nhwc(const float* x, int batch, int c, int hw, const float* scale, const float* shift, void* y,
                        void* stream);
int mvd_op_nhwc_to_nchw(const void* x, int batch, int hw, int c, float* y, void* stream);
int mvd_op_f32_to_bf16(const float* x, int64_t n, void* y, void* stream);
/* One fp32 linear layer of the camera / time MLPs (camera_encoder.py:31-85; diffusers TimestepEmbedding): y[b][o] =
 * sum_k act(x[b][k]) W[o][k] + bias[o]; W fp32 [n][k], or bf16 with wbf16 = 1; act_in = 1 applies SiLU to the inputs. */
int mvd_op_skinny_linear(const float* x, int ldx, int batch, int k, const void* w, int wbf16, const float* bias, int n, int act_in,
                         float* y, int ldy, void* stream);
/* The other kernels of the fp32 camera / time conditioning path, one launcher each.
 * timestep_embedding: y [batch][dim] = [cos | sin] of t * 10000^(-i / (dim/2)), dim even.
 * camera_features: cameras [batch][cam_rows][4] (cam_rows 3 or 4) -> rflat [batch][9] = tR . sR^T, enc [batch][6 nfreq] =
 *   per axis of T = tT - R sT: [sin nfreq | cos nfreq] of T * max_freq^(i / (nfreq - 1)).
 * layernorm_f32: rows of c floats; row r takes gamma / beta + (r % nseg) * c; silu = 1 applies SiLU to the result.
 * skinny_linear_grouped: output feature o of segment g (seg_end[g-1] <= o < seg_end[g], nseg <= 16, even ends, the last = n)
 *   reads the input row x + b * ldx + g * xseg; fp32 weights [n][k], k % 4 == 0.
 * film_params: raw [batch][2 dim] -> scale = 2 strength sigmoid(raw[:dim]), shift = strength raw[dim:], [out_rows][dim] each,
 *   output row r from raw row r % batch.  _grouped: raw [batch][seg_end[nseg-1]] holds 2 dim_g features per segment; segment
 *   g's scale | shift [out_rows][dim_g] start at out + out_rows * seg_end[g-1].
 * im2col_in: x NCHW fp32 (c <= 7), optionally x * scale[b * ld_ss + ch] + shift[b * ld_ss + ch], -> bf16 rows [pixel][64] with
 *   column tap * c + ch of the 3x3 pad-1 window, zero for padding taps and for columns 9 c .. 63.
 * film_nchw_f32: y = x * scale[b][ch] + shift[b][ch] on x [batch][c][hw] fp32. */
int mvd_op_timestep_embedding(const float* t, int batch, int dim, float* y, void* stream);
int mvd_op_camera_features(const float* src, const float* tgt, int batch, int cam_rows, int nfreq, float max_freq, float* rflat,
                           float* enc, void* stream);
int mvd_op_layernorm_f32(const float* x, int rows, int c, float eps, const float* gamma, const float* beta, int silu, int nseg,
                         float* y, void* stream);
int mvd_op_skinny_linear_grouped(const float* x, int ldx, int xseg, int batch, int k, const float* w, const float* bias, int n,
                                 const int* seg_end, int nseg, float* y, int ldy, void* stream);
int mvd_op_film_params(const float* raw, int batch, int dim, float strength, float* scale, float* shift, int out_rows,
                       void* stream);
int mvd_op_film_params_grouped(const float* raw, int batch, const int* seg_end, int nseg, float strength, float* out, int out_rows,
                               void* stream);
int mvd_op_im2col_in(const float* x, int batch, int c, int h, int w, const float* scale, const float* shift, int ld_ss, void* y,
                     void* stream);
int mvd_op_film_nchw_f32(const float* x, int batch, int c, int hw, const float* scale, const float* shift, float* y, void* stream);
int mvd_gemm_num_configs(void);
/* What the calling thread's last GEMM/conv launch did: out[5] = {tile config, split-K, work items, workgroups, workgroups
 * per CU}; last attention launch: out[2] = {waves per workgroup, workgroups}.  Parity tests assert with these that the
 * persistent multi-tile path (work items > workgroups) is what ran at the benchmarked shapes. */
int mvd_debug_last_gemm_plan(int* out);
int mvd_debug_last_attention_plan(int* out);
/* The calling thread's last GroupNorm launch, out[6].  One-pass slice kernel: {1, vectors per thread of the instantiation
 * (2, 4, 8, 16 or 21), threads, groups per workgroup, pixels per pass, 0}; two-kernel form: {2, rows in flight of the
 * statistics kernel, its threads, chunks per image, rows per chunk, rows per block of the apply kernel}. */
int mvd_debug_last_groupnorm_plan(int* out);
/* Launches of the 2x2 sub-pixel upsampling convolution by this process so far (read the difference across a forward). */
long mvd_debug_up4_launches(void);
/* 1 when the calling thread's last small-M split-K launch used the no-wait combine (requested, or chosen because the grid
 * cannot be resident at once), else 0. */
int mvd_debug_last_gemm_nowait(void);
/* The split-K factor the engine's schedule picks for a GEMM/conv of this size (1 = none). */
int mvd_debug_pick_splitk(int m, int n, int k, int geglu);
/* The same for a 3x3 convolution run as an implicit GEMM (k = 9 * Cin + fused shortcut channels). */
int mvd_debug_pick_splitk_conv(int m, int n, int k);
/* The route the engine's single-stream schedule gives a dense GEMM over one or two sources ([a | a2], k1 + k2; k2 = 0: one) with a
 * residual, by host arithmetic alone: out[5] = {1 small-M kernels / 0 tiled kernels, small-M tile / tile config, split-K factor,
 * small-M ring depth (0: tiled), column tiles per group of the 256x320 kernel's tile walk (0: row-major)}.  -1: no dense launch
 * takes the shape (each source width must be a multiple of the 64-deep K slab). */
int mvd_debug_dense_route(int m, int n, int k1, int k2, int* out);
/* 1 when the ping-pong kernel (tile config 7) takes a dense bf16 launch [m][k] . W[n][ldw]^T (+ res[m][ldres]; ldres 0: none) ->
 * out[m][ldo], 0 when it leaves it to the lock-step 256x320 tile, -1 for a bad shape (pure host arithmetic).  Its epilogue moves
 * 16 bytes per access: ldo and ldres must be multiples of 8 elements. */
int mvd_debug_gemm_pp_takes(int m, int n, int k, int ldw, int ldres, int ldo);
/* Small-M kernels (gemm_sm.hip, the batch-1 path): force_cfg = 100 + 10 * tile + ring depth in mvd_op_linear / mvd_op_conv3x3
 * (tiles 0..6 = 64x64, 128x64, 64x128, 128x128, 64x160, 128x160, 64x320; + 1000: the weight is in the blocked LDS-image
 * layout of mvd_amd.packing.block_weight).  With splitk > 1 these kernels combine the slices themselves: splitk_ws then
 * needs splitk*m*n floats + 4096 further 4-byte words (tile arrival counters, zeroed by the call). */
int mvd_gemm_sm_num_tiles(void);
/* Measurement hook: log2(waves per attention workgroup) for every later launch of this process; -1 = heuristic. */
int mvd_debug_set_attention_nw(int nw_log2);
/* Test hooks of the ragged forward.  The two K/V tables the engine builds for view_counts and g rows per view, into host arrays
 * of g * sum(view_counts) entries each (adapter: o * g + j; text: j * objects + o); returns that number of entries, or -1. */
int mvd_debug_ragged_tables(const int* view_counts, int objects, int g, int* adapter, int* text);
/* mvd_op_attention_mapped with a K/V group beside the table: the combination the host rejects (nothing is uploaded or launched). */
int mvd_debug_attention_mapped_grouped(const void* q, const void* k, const void* v, void* o, int batch, int heads, int nq, int nk,
                                       int ldq, int ldk, int ldv, int ldo, float scale, int kv_group, int kv_objects,
                                       const int* kv_index_host, int kv_elements, void* stream);
/* Test hook: ONE attention launch of two problems, exactly as an image-conditioned transformer block issues them (self + reference
 * attention, text + reference cross-attention).  ptrs[8] = {q0, k0, v0, o0, q1, k1, v1, o1} (device); dims[18] = per problem
 * {nq, nk, ldq, ldk, ldv, ldo, kv_group, kv_objects, kv_elements}, batch strides n * ld; table0 / table1: null, or `batch` host
 * entries in [0, kv_elements) of that problem -- checked on the host before anything is uploaded or launched, like a table beside
 * a group.  scale = 0: prescaled queries.  nsplit: 1 = no split-KV, 2..8 = that many key ranges, 0 = the engine's own choice for
 * these arguments.  ws: _ws_bytes(...) bytes of device memory (0: none needed); the call zeroes the arrival counters in it. */
int64_t mvd_debug_attention_pair_ws_bytes(const int* dims, const int* table0, const int* table1, int batch, int heads, float scale,
                                          int nsplit);
int mvd_debug_attention_pair(const void* const* ptrs, const int* dims, const int* table0, const int* table1, int batch, int heads,
                             float scale, int nsplit, void* ws, void* stream);
/* The CLIP towers' and the VAE's own kernels one by one (text.hip, vision.hip, clip_layer.h, vae.hip), each a thin launch of the
 * kernel the tower launches, on caller buffers; tests/test_clip_ops_gpu.py holds them to fp64 references and
 * tests/test_clip_replay_gpu.py composes the towers from them bit for bit.  Every fp32 pointer is 16-byte aligned.
 *
 * Residual add + LayerNorm in one pass: x[rows][H] += delta[rows][H] in place (delta NULL: x is not written), then y = LN(x; gamma,
 * beta, eps) with the two-pass variance, as bf16 (y_bf16) or fp32 (y_f32): exactly one of the two is given.  H % 4 == 0,
 * 4 <= H <= 2048.  clip_layer.h is compiled into both towers' translation units: the two entries reach the two copies. */
int mvd_op_text_add_ln(float* x, const float* delta, const float* gamma, const float* beta, int rows, int H, float eps, void* y_bf16,
                       float* y_f32, void* stream);
int mvd_op_vision_add_ln(float* x, const float* delta, const float* gamma, const float* beta, int rows, int H, float eps, void* y_bf16,
                         float* y_f32, void* stream);
/* The MLP's activation pass, fp32 x[n] -> bf16 y[n]: act 0 gelu (erf form), 1 quick_gelu = x * sigmoid(1.702 x).  n % 8 == 0. */
int mvd_op_text_act(const float* x, int64_t n, int act, void* y_bf16, void* stream);
int mvd_op_vision_act(const float* x, int64_t n, int act, void* y_bf16, void* stream);
/* x[row] = tok[ids[row]] + pos[row % T], rows = batch * T; tok [vocab][H], pos [>= T][H] fp32.  An id outside [0, vocab) is clamped
 * into it (below 0: row 0; vocab and above: row vocab - 1) for address safety only: range validation is the caller's.  H % 4 == 0. */
int mvd_op_text_embed(const int32_t* ids, const float* tok, const float* pos, int rows, int T, int H, int vocab, float* x, void* stream);
/* pixel_values [batch][3][image_size][image_size] fp32 -> bf16 patch rows [batch * (image_size / patch_size)^2][roundup(3 patch_size^2,
 * 64)] in (c, py, px) order, pad columns zero: the rows mvd_vision_encode builds when it is handed pixel_values. */
int mvd_op_vit_patchify(const float* pixel_values, int batch, int image_size, int patch_size, void* patches_bf16, void* stream);
/* x[b][0] = cls + pos[0], x[b][1 + i] = patch_out[b][i] + pos[1 + i], then x = LN(x; gamma, beta, eps) (pre_layrnorm), fp32;
 * patch_out [batch][tokens - 1][H], pos [tokens][H], x [batch][tokens][H].  H as for add_ln. */
int mvd_op_vit_embed_ln(const float* patch_out, const float* cls, const float* pos, const float* gamma, const float* beta, int batch,
                        int tokens, int H, float eps, float* x, void* stream);
/* out[i] = x[i] + delta[i], fp32 (the image tower's last hidden state: the last fc2 result folded into the stream).  n % 4 == 0. */
int mvd_op_vit_fold(const float* x, const float* delta, int64_t n, float* out, void* stream);
/* x[r][:] /= ||x[r]||_2 in place, x [rows][dim] fp32, dim <= 2048: the second launch of mvd_op_clip_pool_project on its own. */
int mvd_op_clip_l2norm(float* x, int rows, int dim, void* stream);
/* quant_conv / post_quant_conv: y[b][o][p] = bias[o] + sum_c w[o][c] x[b][c][p] (fma in channel order), NCHW fp32, hw pixels per
 * plane.  cin, cout <= 8: the kernel keeps a pixel's channels in eight registers, and more is refused before the launch. */
int mvd_op_vae_pointwise(const float* x, int batch, int cin, int cout, int hw, const float* w, const float* bias, float* y, void* stream);
/* Test hooks of the replay tests.  clip_linear: out[M][N] = a[M][K] . w[N][K]^T + bias through the towers' own routing (ClipCtx::linear:
 * the small-M planner with its in-kernel split-K, else the tiled kernels with mvd_gemm_pick_splitk); a, w bf16, out bf16 or
 * (out_f32) fp32; N, K multiples of 64.  ws: _ws_bytes(...) bytes of 256-byte aligned device memory, [split-K tile counters |
 * partials]; the call zeroes the counters as the towers do at the head of an encode.  route_out (nullable, host): {small-M tile, or -1 for
 * the tiled kernels; split-K factor}.  clip_attention: the image tower's
 * attention launch over fused rows qkv [batch * tokens][3 * heads * 64] bf16 (q prescaled) -> out [batch * tokens][heads * 64]. */
int64_t mvd_debug_clip_linear_ws_bytes(int M, int N, int K, int out_f32);
int mvd_debug_clip_linear(const void* a, int K, int M, const void* w, const float* bias, int N, void* out, int out_f32, void* ws,
                          int64_t ws_bytes, int* route_out, void* stream);
int mvd_debug_clip_attention(const void* qkv_bf16, void* out_bf16, int batch, int heads, int tokens, void* stream);
/* Measurement / bisection switches (bench.py --debug-flags, tools/, A/B tests): OR them into mvd_debug_set_flags.  Every switch
 * is read per launch or per forward unless it says otherwise, so 0 restores the product's behaviour.  The values are quoted
 * by DESIGN.md and profiles/ and never change; mvd_amd/_lib.py DebugFlag mirrors them (tests/test_cabi_cpu.py compares). */
typedef enum {
  MVD_DBG_NO_SM_LN_FOLD = 1,            /* no LayerNorm fold through the small-M kernels */
  MVD_DBG_SM_NO_SPLITK = 2,             /* small-M kernels never split K */
  MVD_DBG_NO_SM = 4,                    /* small-M kernels off */
  MVD_DBG_NO_SPLIT_KV = 8,              /* no split-KV attention */
  MVD_DBG_ONE_STREAM = 16,              /* encoder pass on the caller's stream */
  MVD_DBG_SINGLE_STREAM_POLICY = 32,    /* single-stream launch policy (split-K / tile choice) also while two streams run */
  MVD_DBG_SIDE_DEFAULT_PRIORITY = 64,   /* side stream at default instead of highest priority (read when the stream is created) */
  MVD_DBG_NO_XS = 128,                  /* X-stationary kernels off */
  MVD_DBG_NO_WS = 256,                  /* conv_ws off */
  MVD_DBG_WS_SMALL_MAPS = 512,          /* conv_ws only for maps of at most 256 pixels */
  MVD_DBG_WS_BLOCK64 = 1024,            /* conv_ws 64-pixel blocks everywhere */
  MVD_DBG_WS_NO_SHORTCUT = 2048,        /* conv_ws not with a fused shortcut */
  MVD_DBG_WS_NOT_IN_ENCODER = 4096,     /* conv_ws not in the encoder pass of a two-stream forward */
  MVD_DBG_WS_ONLY_IN_ENCODER = 8192,    /* conv_ws only in the encoder pass of a two-stream forward */
  MVD_DBG_WS_THEN_TILED = 16384,        /* conv_ws, and then the tiled kernel over it */
  MVD_DBG_WS_CHECK = 32768,             /* probe builds: compare conv_ws with the tiled kernel */
  MVD_DBG_GRAPH_ONE_STREAM = 65536,     /* graph capture on one stream */
  MVD_DBG_PP_ROW_MAJOR = 131072,        /* ping-pong kernels: row-major tile walk (gemm_pp.hip) */
  MVD_DBG_NO_DEEP_CONV_SPLIT = 262144,  /* no deep-conv split rule (gemm.hip deep_conv_split) */
  MVD_DBG_LATE_FROM_UP1 = 524288,       /* main pass back to the single-stream policy from up_blocks.1 on */
  MVD_DBG_NO_UP4 = 1048576,             /* upsamplers keep the nine-tap kernel (no 2x2 sub-pixel form) */
  MVD_DBG_GN_ONE_PASS = 2097152,        /* one-pass GroupNorm also for few big slices (norm.hip) */
  MVD_DBG_FORK_LATE = 4194304,          /* front matter of both passes first, the stream fork behind it */
  MVD_DBG_SKINNY_VECTOR = 8388608       /* skinny linear: vector form instead of the fp32 matrix pipe (misc.hip) */
} mvd_debug_flag_t;
int mvd_debug_set_flags(int flags);

/* ---- denoising-loop helpers either side of the UNet, fp32 latents ------ */
/* DDPM ancestral step, coefficients from mvd_amd/scheduler.py (diffusers DDPMScheduler.step algebra):
 *   x0 = c0*model_out + c1*sample ; out = c2*x0 + c3*sample + sigma*noise.   Replaces pipeline.py:161. */
int mvd_op_ddpm_step(const float* model_out, const float* sample, const float* noise, float c0, float c1, float c2,
                     float c3, float sigma, float* out, int64_t n, void* stream);
/* classifier-free guidance combine of [uncond | cond] stacked on the batch dim (pipeline.py:156-158) */
int mvd_op_cfg_combine(const float* uncond_cond, float guidance_scale, float* out, int64_t n_half, void* stream);
/* One DDIM / DPM-Solver++ step (mvd_amd/scheduler.py computes the per-step scalars on the host; nothing is uploaded):
 *   m = guided ? u + guidance_scale*(c - u) : model_out   ([uncond | cond] stacked on the batch dim: 2n floats when guided)
 *   x0 = a0*m + a1*sample ; out = p*sample + q*x0 + r*x0_prev + sigma*noise ; if (x0_out) x0_out = x0 (multistep history).
 * x0_prev may be NULL iff r == 0, noise may be NULL iff sigma == 0, n % 4 == 0; otherwise -1 (mvd_last_error).  In place is
 * allowed for out == sample and x0_out == x0_prev (every element is read and then written by the same thread); no other
 * argument may overlap an output. */
int mvd_op_sampler_step(const float* model_out, int guided, float guidance_scale, const float* sample, const float* x0_prev,
                        const float* noise, float a0, float a1, float p, float q, float r, float sigma, float* out,
                        float* x0_out, int64_t n, void* stream);
/* Guidance rescale (Lin et al. 2024, section 3.4; diffusers-0.32.2 rescale_noise_cfg, restated) fused into the guided step.
 * uncond_cond / model_out hold [uncond | cond] stacked on the batch dim: 2 * rows * n_row floats.  Per row, over its n_row
 * elements:  m = u + g*(c - u) ; s_c = std(c), s_m = std(m) (unbiased, divisor n_row - 1) ;
 *            m' = m * (phi * s_c / s_m + 1 - phi)              (= phi * m * s_c / s_m + (1 - phi) * m)
 * mvd_op_cfg_rescale writes out = m'; mvd_op_sampler_step_rescaled goes on as mvd_op_sampler_step does with m' for m:
 *   x0 = a0*m' + a1*sample ; out = p*sample + q*x0 + r*x0_prev + sigma*noise ; if (x0_out) x0_out = x0.
 * ONE launch, one workgroup per row; the two statistics are fp64 sums of x and x^2 taken in a fixed order that depends on
 * n_row alone (no atomics), so a row's output bits do not depend on rows, on the row's index or on the launch.  A row of up
 * to 36864 floats stays in registers between the statistics and the update (model_out is read once); a longer row is read a
 * second time.  There is no epsilon: s_m == 0 gives what IEEE arithmetic gives (inf or NaN), as in diffusers; a variance that
 * rounds below zero counts as zero.  guidance_rescale must lie in [0, 1], n_row % 4 == 0, n_row >= 4; x0_prev / noise as in
 * mvd_op_sampler_step; out == sample and x0_out == x0_prev are allowed; an out or x0_out that overlaps uncond_cond / model_out
 * is an error (every element of a row is needed before any output of it is final); otherwise -1 (mvd_last_error). */
int mvd_op_cfg_rescale(const float* uncond_cond, float guidance_scale, float guidance_rescale, float* out, int64_t rows,
                       int64_t n_row, void* stream);
int mvd_op_sampler_step_rescaled(const float* model_out, float guidance_scale, float guidance_rescale, const float* sample,
                                 const float* x0_prev, const float* noise, float a0, float a1, float p, float q, float r,
                                 float sigma, float* out, float* x0_out, int64_t rows, int64_t n_row, void* stream);
/* How the two entry points above partition a row of n_row floats, out[4] = {threads per workgroup, floats per lane access,
 * lanes per wave, 16-byte vectors per thread kept in registers (0: the row is streamed twice)}: thread t of the row's one
 * workgroup owns the vectors t, t + threads, t + 2*threads, ... of the row. */
int mvd_debug_cfg_rescale_plan(int64_t n_row, int* out);
/* Adaptive projected guidance (Sadat, Hilliges and Weber, ICLR 2025; diffusers' normalized_guidance with
 * use_original_formulation=True, restated) fused into the guided step.  uncond_cond / model_out hold [uncond | cond] stacked on the
 * batch dim: 2 * rows * n_row floats; momentum_buffer M holds rows * n_row floats and is updated in place.  Per row, over its
 * n_row elements, with g = guidance_scale, tau = norm_threshold, beta = momentum, phi = guidance_rescale:
 *   d = (c - u) + beta*M ; M = d                         (fp32, one fma; beta == 0: M is neither read nor written and may be NULL)
 *   s = tau > 0 ? min(1, tau / sqrt(sum d^2)) : 1         (sum d^2 == 0: s = 1)
 *   alpha = sum c^2 > 0 ? s * sum(d c) / sum c^2 : 0      (the coefficient of c in the part of s*d parallel to c)
 *   m = c + (g - 1)*(s*d - (1 - eta)*alpha*c) = A*c + B*d ,  A = 1 - (g - 1)(1 - eta) alpha ,  B = (g - 1) s
 *   phi > 0:  m = m * (phi * std(c) / std(m) + 1 - phi)   (mvd_op_cfg_rescale's rescale: unbiased std, no epsilon)
 * eta = 1, tau = 0, beta = 0, phi = 0 is plain classifier-free guidance.  mvd_op_apg writes out = m.  mvd_op_sampler_step_apg goes
 * on as mvd_op_sampler_step does:  x0 = a0*m + a1*sample ; out = p*sample + q*x0 + r*x0_prev + sigma*noise ; if (x0_out) x0_out = x0.
 * space 0 ("output"): as above, on the model output.  space 1 ("x0", the paper's setting): c = a0*c + a1*sample and d = a0*(c - u)
 * + beta*M first, so the projection, the cap and M live in denoised-prediction space, and m is the step's x0 directly; phi must
 * then be 0.  ONE launch, one workgroup per row; the five statistics (sum c, sum d, sum c^2, sum d^2, sum c d) are fp64 sums in a
 * fixed order that depends on n_row alone (no atomics), and the moments of m follow from them, so a row's output bits do not
 * depend on rows, on the row's index or on the launch.  A row of up to 36864 floats stays in registers between the statistics
 * and the update; a longer row is read a second time (d from M when beta != 0).  eta and phi must lie in [0, 1], tau must be
 * finite and >= 0, beta must lie in (-1, 1), n_row % 4 == 0; M is required when beta != 0; x0_prev / noise as in
 * mvd_op_sampler_step; out == sample and x0_out == x0_prev are allowed; an out, x0_out or M that overlaps the model output, or an M
 * that overlaps any other argument, is an error; otherwise -1 (mvd_last_error), before anything is launched. */
int mvd_op_apg(const float* uncond_cond, float guidance_scale, float eta, float norm_threshold, float momentum,
               float guidance_rescale, float* momentum_buffer, float* out, int64_t rows, int64_t n_row, void* stream);
int mvd_op_sampler_step_apg(const float* model_out, float guidance_scale, float eta, float norm_threshold, float momentum,
                            float guidance_rescale, int space, float* momentum_buffer, const float* sample, const float* x0_prev,
                            const float* noise, float a0, float a1, float p, float q, float r, float sigma, float* out,
                            float* x0_out, int64_t rows, int64_t n_row, void* stream);
/* The partition of a row by the two entry points above, out[4] as mvd_debug_cfg_rescale_plan. */
int mvd_debug_apg_plan(int64_t n_row, int* out);
/* One UniPC step (Zhao et al., NeurIPS 2023; diffusers-0.32.2 UniPCMultistepScheduler with predict_x0, restated; SURVEY.md 8f row
 * N23): the corrector of the previous step and the predictor of this one in ONE launch.  mvd_amd/scheduler.py computes the
 * per-step scalars on the host; nothing is uploaded.  Per element:
 *   m  = guided ? u + guidance_scale*(c - u) : model_out   ([uncond | cond] stacked on the batch dim: 2n floats when guided)
 *   x0 = a0*m + a1*sample                                  (sample: this step's input, the uncorrected prediction)
 *   xc = corr ? cx*last_sample + c0*h0 + c1*h1 + c2*h2 + ct*x0 : sample
 *   out = px*xc + p0*x0 + p1*h0 + p2*h1 ;  if (xc_out) xc_out = xc ;  if (x0_out) x0_out = x0
 * last_sample is the previous step's (corrected) sample, h0, h1, h2 the previous x0 predictions, newest first.  Every operation is
 * one fp32 rounding, in this order: m = fma(c - u, g, u); x0 = fma(a0, m, a1*sample); xc = cx*last_sample, then fma(c0, h0, .),
 * fma(c1, h1, .), fma(c2, h2, .), fma(ct, x0, .); out = px*xc, then fma(p0, x0, .), fma(p1, h0, .), fma(p2, h1, .).  A term whose
 * coefficient is 0 is skipped and its pointer, which may be NULL, is never read; corr == 0 zeroes cx .. ct.  n % 4 == 0;
 * last_sample is required with corr; h0 when c0 != 0 or p1 != 0, h1 when c1 != 0 or p2 != 0, h2 when c2 != 0.  In place is allowed
 * for out == sample, xc_out == last_sample and x0_out == any one of h0 .. h2 (every element is read and then written by the same
 * thread); an output that overlaps model_out or another output is an error; otherwise -1 (mvd_last_error), before anything is
 * launched.  The history rotates on the host by rotating buffer roles: the kernel writes only the newest x0. */
int mvd_op_unipc_step(const float* model_out, int guided, float guidance_scale, const float* sample, const float* last_sample,
                      const float* h0, const float* h1, const float* h2, float a0, float a1, int corr, float cx, float c0, float c1,
                      float c2, float ct, float px, float p0, float p1, float p2, float* out, float* xc_out, float* x0_out, int64_t n,
                      void* stream);

/* FreeU on the two inputs of an up-block resnet, ONE launch.  hidden [B][H*W][C] and skip [B][H*W][Cs] are bf16, token-major:
 *   hidden_out = hidden with channels [0, C / 2) multiplied by b (fp32 product, one rounding to bf16), the rest bit for bit;
 *   skip_out   = skip with the spatial frequencies {0, -1} x {0, -1} of every (image, channel) map multiplied by s -- diffusers'
 *                fourier_filter with threshold 1 -- as the closed form
 *                  x + (s - 1) / (H W) * sum_{k,l in {0,1}} (a_kl cos phi_kl + b_kl sin phi_kl),  phi_kl = 2 pi (k h / H + l w / W),
 *                a_kl / b_kl the cosine / sine sums of the map: fp32 sums in a fixed order (no atomics: the same bits every
 *                run), the formula in fp32, one rounding to bf16.  s == 1 copies the skip map bit for bit.
 * -1 (mvd_last_error), before anything is launched, for H or W < 2, C or Cs no positive multiple of 8, b or s not positive and
 * finite, a pointer that is null or not 16-byte aligned, or an output that overlaps an input or the other output. */
int mvd_op_freeu(const void* hidden, int C, const void* skip, int Cs, int B, int H, int W, float b, float s, void* hidden_out,
                 void* skip_out, void* stream);

/* Token merging (Bolya & Hoffman 2023; tomesd 0.1.x with use_rand = False, sx = sy = 2, restated) on a token-major bf16 map
 * x [B][H*W][C], every image on its own.  dst tokens: the top-left token of every complete 2 x 2 cell, nd = (H/2)(W/2), numbered in
 * raster order of the cells; src tokens: every other token (a last odd row / column included), ns = H W - nd, numbered in ascending
 * token order.  score(s, d) = x_s . x_d / (|x_s| |x_d|): exact bf16 products, fp32 sums, the division on the fp32 result;
 * best(s) = argmax over d, a tie to the lowest d.  The r src with the largest score(s, best(s)) are merged, ties to the lower index.
 *   mvd_op_tome_match        slot [B][H W] int32: the row of every token in the merged sequence of N' = H W - r rows (dst d -> d, a
 *                            merged src -> best(s), the p-th kept src in ascending token order -> nd + p); members [B][H W] and
 *                            starts [B][N' + 1] int32: the tokens of row j are members[starts[j] .. starts[j + 1]), ascending.
 *                            score / best [B][ns] (fp32 / int32) may be null: they then live in ws (mvd_op_tome_workspace_bytes,
 *                            256-byte aligned).  Two launches (match, select); nothing is synchronised.
 *   mvd_op_tome_merge        out [B][N'][C] = bf16(fp32 sum of the row's members in ascending token order / count); a row of one
 *                            member is copied bit for bit.
 *   mvd_op_tome_unmerge_add  h [B][H W][C] += t [B][N'][C] rows by slot, in place: bf16(float(h) + float(t)).
 * -1 (mvd_last_error) before anything is launched for H or W < 2, H W above the select kernel's limit (mvd_debug_tome_plan out[7]),
 * C no positive multiple of 64, r outside [0, ns], a null or misaligned pointer.
 * mvd_debug_tome_plan: out[8] = nd, ns, N', score sort keys, member sort keys, match workgroups per image, select LDS bytes, the
 * token limit (out[7] is written even when the shape is refused). */
int64_t mvd_op_tome_workspace_bytes(int B, int H, int W);
int mvd_op_tome_match(const void* x, int B, int H, int W, int C, int r, int* slot, int* members, int* starts, float* score_or_null,
                      int* best_or_null, void* ws, int64_t ws_bytes, void* stream);
int mvd_op_tome_merge(const void* x, int B, int H, int W, int C, int r, const int* members, const int* starts, void* out, void* stream);
int mvd_op_tome_unmerge_add(void* h, const void* t, int B, int H, int W, int C, int r, const int* slot, void* stream);
int mvd_debug_tome_plan(int H, int W, int C, int r, int64_t* out);

/* Token downsampling (ToDo, restated) of K and V rows: k and v point at the K and V columns of token-major bf16 rows
 * [B][H*W] that share the row stride ld (elements; the fused q/k/v buffer: 3C or 4C) and the batch stride H W ld.  The key map is
 * Hk x Wk = (H / f) x (W / f); tokens of an incomplete last row or column of cells are in no key.
 *   method 0 (nearest)  key (i, j) = the row of token (i f, j f), bit for bit
 *   method 1 (area)     key (i, j) = bf16(fp32 sum of the cell's f*f rows in row-major order / float(f*f)), RNE
 * out [B][Hk Wk][2C] bf16: K in columns [0, C), V in [C, 2C).  One launch.  -1 (mvd_last_error) before it for f outside {2, 3, 4},
 * a method outside {0, 1}, C no positive multiple of 8, ld no multiple of 8 or below C, a null or not 16-byte aligned pointer,
 * H / f or W / f = 0, or out overlapping the input rows. */
int mvd_op_todo_downsample(const void* k, const void* v, int ld, int B, int H, int W, int C, int f, int method, void* out, void* stream);

/* ---- checkpoint scoring around the UNet, fp32 ------------------------------------------------ */
/* Conventions of the helpers above; in addition every quantity that depends on a sample's timestep is read ON THE DEVICE
 * from fp32 tables of num_train_timesteps entries indexed by the int32 device vector timesteps[batch] (clamped to the table
 * for address safety only: range checks are the caller's), so nothing is uploaded per call.  Reductions are fixed-order
 * (one partial per workgroup in the caller's workspace, summed in index order by a finalize kernel; no float atomics):
 * two launches on the same input give the same bits.  Inputs and outputs must not overlap.
 *
 * Forward diffusion of x0[batch][per_sample] (diffusers' add_noise / get_velocity; training.py:208, losses.py:168):
 *   noisy = a x0 + s noise ; velocity = a noise - s x0 ; a = sqrt_ac[t_b], s = sqrt_1mac[t_b].  Either output may be NULL
 * (not both); per_sample % 4 == 0, batch <= 65535. */
int mvd_op_add_noise(const float* x0, const float* noise, const int32_t* timesteps, const float* sqrt_ac, const float* sqrt_1mac,
                     int num_train_timesteps, float* noisy, float* velocity, int batch, int64_t per_sample, void* stream);
/* The forward-only core of compute_losses (losses.py:128-238) in one pass over (pred, noise, x0, noisy):
 *   prediction_type 0 epsilon:      target = noise ;            denoised = (noisy - s pred) / a
 *                   1 v_prediction: target = a noise - s x0 ;   denoised = a noisy - s pred
 *                   2 sample:       target = x0 ;               denoised = pred
 *   result[0] = mse = mean (pred - target)^2            result[1] = mse * mean_b w_b,  w_b = min(snr_b, snr_gamma) / snr_b
 *   result[2] = mean (denoised - x0)^2                  result[3] = mean_b snr_b       result[4] = mean_b w_b
 * with snr_b = snr[t_b] (a table of its own: the reference takes it from another scheduler object than a and s).  x0 may be
 * NULL for epsilon; without x0 and noisy (noisy is not read for sample) result[2] = 0 and `denoised` must be NULL; otherwise
 * `denoised`, when given, receives the denoised latents.  Workspace: the _ws_bytes function below, or more. */
int64_t mvd_op_noise_loss_ws_bytes(int batch, int64_t per_sample);
int mvd_op_noise_loss(const float* pred, const float* noise, const float* x0, const float* noisy, const int32_t* timesteps,
                      const float* sqrt_ac, const float* sqrt_1mac, const float* snr, int num_train_timesteps, int prediction_type,
                      float snr_gamma, float* denoised, float* result, int batch, int64_t per_sample, void* ws, int64_t ws_bytes,
                      void* stream);
/* Mean squared error and, with want_ssim, SSIM of two NCHW batches x, y [n][c][h][w] from one read of both:
 *   result[0] = mse over all elements   result[1] = SSIM (0 without want_ssim)   result[2] = PSNR = 10 log10(R^2 / mse)
 *   per_image (may be NULL) [n][2] = each image's (mse, SSIM); their means over n are result[0], result[1].
 * R = data_range.  SSIM is pytorch_msssim 1.0.0 with its defaults: 11-tap Gaussian window (sigma 1.5, sum 1) applied
 * separably without padding to x, y, x^2, y^2, x y; C1 = (0.01 R)^2, C2 = (0.03 R)^2; the map's mean per (image, channel),
 * then the mean of those.  PSNR is torchmetrics' PeakSignalNoiseRatio(data_range=R) (+inf on identical inputs).
 * Any c, any h, w >= 11 (smaller: -1, never an unfiltered comparison); n c h w < 2^31. */
int64_t mvd_op_image_metrics_ws_bytes(int n, int c, int h, int w, int want_ssim);
int mvd_op_image_metrics(const float* x, const float* y, int n, int c, int h, int w, float data_range, int want_ssim, float* result,
                         float* per_image, void* ws, int64_t ws_bytes, void* stream);

/* ---- AutoencoderKL (SD-2.1 VAE) either side of the loop ------------------------------------ */
/* Replaces: vae.encode(x).latent_dist (pipeline.py:115) and vae.decode(z).sample (pipeline.py:171-176) of diffusers'
 * AutoencoderKL.  Slot names / layouts: DESIGN.md "VAE weight slots" (mvd_amd/vae.py packs a diffusers state dict). */
typedef struct {
  int in_channels;                         /* 3 */
  int latent_channels;                     /* 4 */
  int num_levels;                          /* 4 */
  int block_out_channels[MVD_MAX_LEVELS];  /* 128 256 512 512 */
  int layers_per_block;                    /* 2 */
  int norm_num_groups;                     /* 32 */
  float norm_eps;                          /* 1e-6 */
} mvd_vae_config_t;
typedef struct mvd_vae mvd_vae_t;
int mvd_vae_create(const mvd_vae_config_t* cfg, mvd_vae_t** out);
int mvd_vae_destroy(mvd_vae_t* v);
int mvd_vae_set_weight(mvd_vae_t* v, const char* slot, const void* ptr, int64_t numel, int dtype);
/* bytes for one encode (decode = 0: height/width of the IMAGE) or decode (decode = 1: height/width of the LATENT) */
int64_t mvd_vae_workspace_bytes(mvd_vae_t* v, int batch, int height, int width, int decode);
int mvd_vae_bind_workspace(mvd_vae_t* v, void* ws, int64_t ws_bytes);
/* image [batch][in_channels][H][W] fp32 in [-1,1] -> moments [batch][2*latent][H/f][W/f] fp32 = (mean | logvar) */
int mvd_vae_encode(mvd_vae_t* v, const float* image_nchw, int batch, int height, int width, float* moments, void* stream);
/* latents [batch][latent][h][w] fp32 (already divided by the scaling factor) -> image [batch][in_channels][f*h][f*w] fp32 */
int mvd_vae_decode(mvd_vae_t* v, const float* latents_nchw, int batch, int height, int width, float* image, void* stream);
/* One mid-block attention (GroupNorm, q / k / v, softmax(q.k^T / sqrt(C)).v, out-projection + residual) of the encoder
 * (decoder = 0) or the decoder (decoder = 1), with the weights set on v, on caller buffers: x, out [batch][height][width][C]
 * bf16 NHWC, C = the deepest level's channel count; height * width must be a multiple of 64.  The same code as inside
 * mvd_vae_encode / mvd_vae_decode.  Checks the bound workspace before it launches anything. */
int64_t mvd_vae_mid_attention_workspace_bytes(mvd_vae_t* v, int decoder, int batch, int height, int width);
int mvd_vae_mid_attention(mvd_vae_t* v, int decoder, const void* x_nhwc_bf16, int batch, int height, int width, void* out_nhwc_bf16,
                          void* stream);
/* The attention's row softmax: p[r][i] = exp(s[r][i] - max_r) / sum_r, fp32 scores [rows][n] -> bf16 probabilities */
int mvd_op_softmax_rows(const float* s, int rows, int n, void* p_bf16, void* stream);
/* DiagonalGaussianDistribution.sample(): out = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scale; noise/out [batch][c][hw] */
int mvd_op_gaussian_sample(const float* moments, const float* noise, int batch, int channels, int hw, float scale, float* out,
                           void* stream);

/* ---- CLIP text encoder in front of the loop ------------------------------------------------ */
/* Replaces: text_encoder(tokenizer(prompt).input_ids)[0] of transformers' CLIPTextModel (pipeline.py:52-75): the
 * last_hidden_state only (no pooler, no attention mask: the reference passes input_ids alone, pipeline.py:62, 72).
 * SD-2.1 values in comments.  Slot names / layouts: DESIGN.md "Text-encoder weight slots" (mvd_amd/text_encoder.py packs a
 * transformers state dict). */
typedef struct {
  int vocab_size;          /* 49408 */
  int hidden_size;         /* 1024 */
  int intermediate_size;   /* 4096 */
  int num_layers;          /* 23 */
  int num_heads;           /* 16 (head dimension 64) */
  int max_positions;       /* 77 */
  float layer_norm_eps;    /* 1e-5 */
  int act;                 /* 0 gelu (erf), 1 quick_gelu = x * sigmoid(1.702 x) */
} mvd_text_config_t;
typedef struct mvd_text mvd_text_t;
/* rejects hidden_size / num_heads != 64, hidden_size % 64 (or > 2048), intermediate_size % 64, max_positions > 96, an unknown act */
int mvd_text_create(const mvd_text_config_t* cfg, mvd_text_t** out);
int mvd_text_destroy(mvd_text_t* t);
int mvd_text_set_weight(mvd_text_t* t, const char* slot, const void* ptr, int64_t numel, int dtype);
int64_t mvd_text_workspace_bytes(mvd_text_t* t, int batch, int seq_len);
int mvd_text_bind_workspace(mvd_text_t* t, void* ws, int64_t bytes);
/* ids [batch][seq_len] int32 (clamped into the vocabulary for address safety only: validate on the host) ->
 * out [batch][seq_len][hidden_size] fp32.  A missing weight slot, an unbound or too small workspace and seq_len >
 * max_positions return < 0 before anything is launched.  No allocation, no host synchronisation; everything on `stream`. */
int mvd_text_encode(mvd_text_t* t, const int32_t* ids, int batch, int seq_len, float* out, void* stream);
/* The encoder's attention (CLIPAttention with the causal mask of CLIPTextTransformer, reached through pipeline.py:62, 72):
 * softmax(scale * q.k^T + causal).v per head of 64 channels, nq == nk == n <= 96, key j visible to query i iff j <= i; one
 * workgroup per (batch, head) with the whole problem in LDS.  scale == 0: q is prescaled by scale * log2(e), as for
 * mvd_op_attention.  q / k / v 16-byte aligned with row strides that are multiples of 8 (views of one fused QKV buffer). */
int mvd_op_attention_causal(const void* q, const void* k, const void* v, void* o, int batch, int heads, int n, int ldq, int ldk,
                            int ldv, int ldo, float scale, void* stream);

/* ---- CLIP image tower and CLIP score for checkpoint validation ------------------------------ */
/* Replaces: the CLIP half of torchmetrics' CLIPScore / transformers' CLIPModel + CLIPImageProcessor as the reference's
 * validation uses them (val.py:60-196, losses.py:59-98): image preprocessing, get_image_features, the pooled and
 * projected text features, and the cosine.  ViT-L/14 values in comments.  Slot names / layouts: DESIGN.md "Vision-encoder
 * weight slots" (mvd_amd/vision_encoder.py packs a transformers state dict). */
typedef struct {
  int image_size;          /* 224 */
  int patch_size;          /* 14: 256 patches + the class token = 257 tokens */
  int hidden_size;         /* 1024 */
  int intermediate_size;   /* 4096 */
  int num_layers;          /* 24 */
  int num_heads;           /* 16 (head dimension 64) */
  int projection_dim;      /* 768 */
  float layer_norm_eps;    /* 1e-5 */
  int act;                 /* 0 gelu (erf), 1 quick_gelu = x * sigmoid(1.702 x) */
} mvd_vision_config_t;
typedef struct mvd_vision mvd_vision_t;
/* rejects hidden_size / num_heads != 64, hidden_size % 64 (or > 2048), intermediate_size % 64, projection_dim % 64 (or > 2048),
 * image_size % patch_size, an unknown act */
int mvd_vision_create(const mvd_vision_config_t* cfg, mvd_vision_t** out);
int mvd_vision_destroy(mvd_vision_t* v);
int mvd_vision_set_weight(mvd_vision_t* v, const char* slot, const void* ptr, int64_t numel, int dtype);
/* bytes for preprocessing `batch` images of h x w (resize_to: the shortest edge after the resize) and encoding them;
 * h = w = 0: encode only.  The workspace holds [resampling tables | bf16 patch rows | scratch]. */
int64_t mvd_vision_workspace_bytes(mvd_vision_t* v, int batch, int h, int w, int resize_to);
int mvd_vision_bind_workspace(mvd_vision_t* v, void* ws, int64_t bytes);
/* CLIPImageProcessor on the device.  images [batch][3][h][w] fp32: in [-1, 1] with quantize = 1, where the first step is
 * ((x.clamp(-1, 1) + 1) / 2 * 255).to(uint8) of losses.py:11-13 (the same fp32 operations, truncation), or integral values in
 * [0, 255] with quantize = 0.  Then PIL's 8-bit BICUBIC Image.resize to the shortest-edge size (resize_to, int(resize_to *
 * long / short)) -- a horizontal and a vertical pass in 2^22 fixed point, each rounded to uint8, a pass between equal sizes
 * skipped: integer arithmetic, so the result equals PIL's byte for byte -- the centre crop (top = (oh - crop) / 2, left alike),
 * u8 / 255 and (x - mean) / std.  want_patches: bf16 patch rows [batch * (crop / patch)^2][roundup(3 patch^2, 64)] in (c, py,
 * px) order with zero pad columns stay in the workspace for mvd_vision_encode (crop must be the model's image_size);
 * pixel_values (nullable) [batch][3][crop][crop] fp32 is what the processor returns.  The coefficient tables are built on the
 * host once per (h, w, resize_to) and uploaded on the first call of that geometry on the bound workspace; later calls upload
 * nothing.  A resized image smaller than the crop is an error (no padding).  No allocation, no host synchronisation. */
int mvd_vision_preprocess(mvd_vision_t* v, const float* images_nchw, int batch, int h, int w, int quantize, int resize_to, int crop,
                          const float* mean, const float* std_, int want_patches, float* pixel_values, void* stream);
/* byte offset in the bound workspace of the patch rows the last mvd_vision_preprocess(want_patches) left there ([batch *
 * patches][Kp] bf16), < 0 when there are none: lets a test read what the encoder will read */
int64_t mvd_vision_patch_rows_offset(mvd_vision_t* v);
/* pixel_values [batch][3][image_size][image_size] fp32, or NULL: the patch rows the last mvd_vision_preprocess(want_patches)
 * of the same batch left in the workspace.  last_hidden_out (nullable) [batch][tokens][hidden_size]: the encoder output
 * before post_layernorm (transformers' last_hidden_state); embeds_out / embeds_norm_out (either nullable) [batch][projection_dim]:
 * visual_projection(post_layernorm(token 0)) -- get_image_features -- and the same rows L2-normalised.  A missing weight slot
 * and an unbound or too small workspace return < 0 before anything is launched.  No allocation, no host synchronisation;
 * everything on `stream`. */
int mvd_vision_encode(mvd_vision_t* v, const float* pixel_values, int batch, float* last_hidden_out, float* embeds_out,
                      float* embeds_norm_out, void* stream);
/* One pooled row per batch element -> [LayerNorm] -> bias-free projection proj_w [proj_dim][hidden_size] fp32 (fp32
 * accumulation) -> embeds (raw) and embeds_norm (divided by the L2 norm); either output nullable.  row = hidden[b][tok]
 * (+ delta[b][tok] when delta is given).  ids NULL: tok = 0 (the image tower: give post_layernorm as ln_gamma / ln_beta).  ids
 * [batch][tokens] int32 (the text tower: hidden = mvd_text_encode's output, already behind final_layer_norm, ln NULL): tok =
 * the argmax of the ids when eos_token_id == 2 (transformers' legacy rule), else the first position equal to eos_token_id
 * (0 when there is none), found on the device.  Two launches: one workgroup per (row, 64 output features), then the L2
 * normalisation of embeds_norm in place (skipped without it).  hidden_size % 4 == 0; hidden_size, proj_dim <= 2048. */
int mvd_op_clip_pool_project(const float* hidden, const float* delta, const int32_t* ids, int batch, int tokens, int hidden_size,
                             int eos_token_id, const float* ln_gamma, const float* ln_beta, float eps, const float* proj_w, int proj_dim,
                             float* embeds, float* embeds_norm, void* stream);
/* per_row_out[b] = sum_c a[b][c] b[b][c] and mean_out[0] = their mean (either nullable): the cosine of L2-normalised rows.
 * One workgroup, sums in a fixed order, the mean finished in fp64: two launches give the same bits.  The caller applies
 * CLIPScore's 100 x and max(., 0). */
int mvd_op_clip_cosine(const float* a, const float* b, int batch, int dim, float* per_row_out, float* mean_out, void* stream);

/* ---- VGG-16 perceptual loss for checkpoint validation --------------------------------------- */
/* Replaces: PerceptualLoss of the reference (src/training/losses.py:21-56): torchvision's vgg16().features[:29] on both image
 * batches and the mean squared difference of the two conv5_3 maps.  Thirteen 3x3 pad-1 convolutions (features.0, 2, 5, 7, 10,
 * 12, 14, 17, 19, 21, 24, 26, 28) with a ReLU behind all but the last, 2x2 max-pools at features.4, 9, 16, 23.
 * Weight slots: "features.N.weight" bf16 in the packed conv layout [cout][cin/64][ky][kx][64] ("features.0.weight": [64][64],
 * column tap * 3 + channel, zero padded from 27), "features.N.bias" fp32 [cout] (mvd_amd/perceptual.py packs a torchvision state
 * dict).  A slot that is missing when a pass runs is error -10, one of another dtype or size -11. */
typedef struct mvd_vgg mvd_vgg_t;
int mvd_vgg_create(mvd_vgg_t** out);
int mvd_vgg_destroy(mvd_vgg_t* v);
int mvd_vgg_set_weight(mvd_vgg_t* v, const char* slot, const void* ptr, int64_t numel, int dtype);
/* bytes for one feature pass over `images` images of h x w (a loss pass over images / 2 pairs), the internal fp32 feature
 * buffer included; found by a dry run of the schedule.  h, w >= 16; images * h * w must stay below 2^31 rows. */
int64_t mvd_vgg_workspace_bytes(mvd_vgg_t* v, int images, int h, int w);
int mvd_vgg_bind_workspace(mvd_vgg_t* v, void* ws, int64_t bytes);
/* images_nchw [images][3][h][w] fp32 in [-1, 1], as PerceptualLoss receives them: (x + 1) / 2, then Normalize(ImageNet mean,
 * std), folded into one affine map per channel in front of conv1_1 (the padding of conv1_1 stays zero).  feat_out_nhwc [images]
 * [h / 16][w / 16][512] fp32: features.28's output, not rounded to bf16.  taps: NULL, or four nullable bf16 NHWC buffers that
 * receive relu1_2 [images][h][w][64], relu2_2 [h/2][w/2][128], relu3_3 [h/4][w/4][256], relu4_3 [h/8][w/8][512] -- the maps in
 * front of the pools.  Pools drop an odd trailing row / column.  No allocation, no host synchronisation; everything on `stream`. */
int mvd_vgg_features(mvd_vgg_t* v, const float* images_nchw, int images, int h, int w, float* feat_out_nhwc, void* const* taps, void* stream);
/* loss_out[0] = mean over pairs and elements of (f(x) - f(y))^2, per_pair_out[p] (nullable) = the mean of pair p; x, y [pairs][3]
 * [h][w] fp32 in [-1, 1].  As many pairs per pass as the bound workspace holds (one pair must fit: -4 otherwise); x and y of a
 * pair are rows of the same launches, so x == y gives exactly 0.  Sums in fp64 in a fixed order: two calls, same bits. */
int mvd_vgg_perceptual(mvd_vgg_t* v, const float* x, const float* y, int pairs, int h, int w, float* loss_out, float* per_pair_out, void* stream);
/* The tower's operators one by one.  conv3x3_relu: mvd_op_conv3x3 restricted to stride 1, no shortcut, row vector or residual,
 * plus relu (out = max(acc + bias, 0) before the one rounding) and out_f32, on the lock-step tiles only (force_cfg -1, 2..5,
 * 10..13; relu = 1: tiles 3, 4, 5 / 11, 12, 13); splitk > 1 needs splitk * M * cout floats of splitk_ws.  linear_relu: the same
 * epilogue behind a dense out[m][n] = a[m][k] . w[n][k]^T + bias (k, n multiples of 64). */
int mvd_op_conv3x3_relu(const void* x, int batch, int in_h, int in_w, int cin, const void* w, const float* bias, void* out, int cout, int relu,
                        int out_f32, int force_cfg, int splitk, float* splitk_ws, void* stream);
int mvd_op_linear_relu(const void* a, int k, const void* w, const float* bias, void* out, int m, int n, int relu, int out_f32, int force_cfg,
                       int splitk, float* splitk_ws, void* stream);
/* NHWC bf16 [batch][h][w][c] -> [batch][h / 2][w / 2][c], 2x2 windows, stride 2 (floor); c a multiple of 8 */
int mvd_op_maxpool2x2(const void* x, int batch, int h, int w, int c, void* y, void* stream);
/* a, b [pairs][n] fp32 (n a multiple of 4): per_pair_out[p] = mean_i (a[p][i] - b[p][i])^2, mean_out[0] = the mean over everything
 * (either nullable).  fp64 sums in a fixed order, no atomics.  ws: the bytes the _ws_bytes query gives, 256-byte aligned. */
int64_t mvd_op_sqdiff_mean_ws_bytes(int pairs, int64_t n);
int mvd_op_sqdiff_mean(const float* a, const float* b, int pairs, int64_t n, float* mean_out, float* per_pair_out, void* ws, int64_t ws_bytes,
                       void* stream);

/* ---- LPIPS v0.1 for checkpoint validation ---------------------------------------------------- */
/* Replaces: lpips.LPIPS(net="alex") of the reference's val.py:87.  The tower is torchvision's alexnet().features[:12]: conv
 * 3->64 11x11 stride 4 pad 2 (features.0), conv 64->192 5x5 pad 2 (features.3), conv 192->384, 384->256, 256->256 3x3 pad 1
 * (features.6, .8, .10), a ReLU behind each (the five taps), a 3x3 stride-2 max-pool behind the first two.  In front of it the
 * scaling layer (x - shift) / scale, shift (-.030, -.088, -.188), scale (.458, .448, .450); behind it, per tap, the maps divided
 * by their channel norm (+ 1e-10), the squared difference weighted by lin_k >= 0, the mean over pixels; the sum over the taps.
 * Weight slots: "features.0.weight" bf16 [64][384], column (ky * 11 + kx) * 3 + c, zero padded from 363; "features.3.weight"
 * bf16 [192][1600], column (ky * 5 + kx) * 64 + c; "features.{6,8,10}.weight" bf16 in the packed conv layout [cout][cin/64]
 * [ky][kx][64]; "features.N.bias" fp32 [cout]; "lin{0..4}.weight" fp32 [C] (mvd_amd/lpips.py packs torchvision / lpips state
 * dicts).  A slot that is missing when a pass runs is error -10, one of another dtype or size -11; nothing is launched then. */
typedef struct mvd_lpips mvd_lpips_t;
int mvd_lpips_create(mvd_lpips_t** out);
int mvd_lpips_destroy(mvd_lpips_t* v);
int mvd_lpips_set_weight(mvd_lpips_t* v, const char* slot, const void* ptr, int64_t numel, int dtype);
/* bytes for one pass over `images` images of h x w (a distance pass over images / 2 pairs), the five taps and the head's partial
 * sums included; found by a dry run of the schedule (no GPU needed); never smaller than the bytes of a pass over fewer images of the
 * same size.  h, w >= 31: below that the second pool has no output. */
int64_t mvd_lpips_workspace_bytes(mvd_lpips_t* v, int images, int h, int w);
int mvd_lpips_bind_workspace(mvd_lpips_t* v, void* ws, int64_t bytes);
/* images_nchw [images][3][h][w] fp32 in [-1, 1].  taps: five bf16 NHWC buffers (an entry may be NULL: that map stays in the
 * workspace) for the post-ReLU maps [images][h1][w1][64], [h2][w2][192], [h3][w3][384], [h3][w3][256], [h3][w3][256] with
 * h1 = (h - 7) / 4 + 1, h2 = (h1 - 3) / 2 + 1, h3 = (h2 - 3) / 2 + 1 -- the maps in front of the pools.  No allocation, no host
 * synchronisation; everything on `stream`. */
int mvd_lpips_features(mvd_lpips_t* v, const float* images_nchw, int images, int h, int w, void* const* taps, void* stream);
/* per_pair_out[p] = d(x[p], y[p]); per_layer_out (nullable) [pairs][5] = the five terms of each; mean_out (nullable) = the mean
 * over the pairs (one of per_pair_out / mean_out must be given); x, y [pairs][3][h][w] fp32 in [-1, 1].  max_pairs_per_pass pairs
 * per pass (<= 0: no cap), fewer where the bound workspace holds fewer (one pair must fit: -4 otherwise); every pass that will run,
 * the shorter last one included, is sized by a dry run before anything is launched.  The pass size decides the split-K of the
 * convolutions and with it the last bits of the result: give the same cap to get the same bits.  x and y of a pair are rows of
 * the same launches, so x == y gives exactly 0.  Sums in fp64 in a fixed order: two calls, same bits. */
int mvd_lpips_distance(mvd_lpips_t* v, const float* x, const float* y, int pairs, int h, int w, int max_pairs_per_pass, float* per_pair_out,
                       float* per_layer_out, float* mean_out, void* stream);
/* The new operators one by one.  im2col_patch, form 0: src fp32 NCHW [batch][3][h][w] -> rows [batch * oh * ow][384] bf16 of the
 * 11x11 stride-4 pad-2 windows, oh = (h - 7) / 4 + 1, column (ky * 11 + kx) * 3 + c, columns 363.. zero; scale / shift: HOST
 * arrays of three floats (both or neither), applied as x * scale[c] + shift[c] to in-image taps only.  Form 1: src bf16 NHWC
 * [batch][h][w][64] -> rows [batch * h * w][1600] of the 5x5 pad-2 windows, column (ky * 5 + kx) * 64 + c (no affine map). */
int mvd_op_im2col_patch(const void* src, int form, int batch, int h, int w, const float* scale, const float* shift, void* rows_out, void* stream);
/* NHWC bf16 [batch][h][w][c] -> [batch][(h - 3) / 2 + 1][(w - 3) / 2 + 1][c], 3x3 windows, stride 2, no padding (floor); c a
 * multiple of 8, h, w >= 3 */
int mvd_op_maxpool3x3s2(const void* x, int batch, int h, int w, int c, void* y, void* stream);
/* The LPIPS head over `layers` <= 8 layers in ONE launch (+ a one-workgroup finish).  Layer l: x[l], y[l] [pairs][pixels[l]]
 * [channels[l]] of dtype[l] (1 bf16, 0 fp32; relu_in[l] = 1 applies max(., 0) to an fp32 map on the way in), lin_w[l] fp32
 * [channels[l]] >= 0; channels a multiple of 64.  per_pair_out[p] = sum_l mean_pixels sum_c w_c (x_c / |x| - y_c / |y|)^2,
 * per_layer_out (nullable) [pairs][layers] the terms, mean_out (nullable) the mean over pairs.  A pixel of zeros on both sides
 * contributes exactly 0.  fp64 sums in a fixed order, no atomics.  ws: the bytes the _ws_bytes query gives, 256-byte aligned. */
int64_t mvd_op_lpips_head_ws_bytes(int layers, const int* pixels, int pairs);
int mvd_op_lpips_head(int layers, const void* const* x, const void* const* y, const int* dtype, const int* relu_in, const int* pixels, const int* channels,
                      const float* const* lin_w, int pairs, float* per_pair_out, float* per_layer_out, float* mean_out, void* ws, int64_t ws_bytes,
                      void* stream);

/* ---- FID: Inception-v3 pool3 features and their statistics, for checkpoint validation ---------- */
/* Replaces: the network inside torchmetrics' FrechetInceptionDistance(feature=2048) of the reference's val.py -- the FID variant
 * of Inception-v3 (torch-fidelity's FeatureExtractorInceptionV3, pytorch-fid's pt_inception-2015-12-05) up to pool3.
 * The layer table lives in ONE place, mvd_amd/packing.py INCEPTION_FID_LAYERS; mvd_fid_create receives it compiled into a
 * program: n_ops records of 13 ints {kind (0 conv, 1 3x3 pool), src buffer, dst buffer, c_off (first channel written in dst),
 * cin (all channels of src), cout, kh, kw, stride, pad_h, pad_w, conv index (0, 1, ... in program order), pool mode}; n_buffers
 * records {channels, is_fp32}: buffer 0 is the front end's output (299 x 299, 16 channels: r, g, b, zeros), final_buffer the fp32
 * map whose mean over the pixels is the feature vector (channels a multiple of 64).  conv_names[k]: convolution k reads the
 * weight slots "<name>.weight" bf16 [cout][kh kw][cin rounded up to 32] (BatchNorm folded, the padding zeros) and "<name>.bias"
 * fp32 [cout].  max_images_per_pass (0: 8) is the pass size: more images run as several passes within one call, whatever earlier
 * calls left bound.  K is never split and its order is fixed: an image's features do not depend on the batch it is part of. */
typedef struct mvd_fid mvd_fid_t;
int mvd_fid_create(const int* program, int n_ops, const int* buffers, int n_buffers, const char* const* conv_names, int n_convs, int final_buffer,
                   int max_images_per_pass, mvd_fid_t** out);
int mvd_fid_destroy(mvd_fid_t* v);
int mvd_fid_set_weight(mvd_fid_t* v, const char* slot, const void* ptr, int64_t numel, int dtype);
int mvd_fid_feature_dim(mvd_fid_t* v);
/* bytes for a call over `images` images of any size (the tower always runs at 299 x 299): a dry run of the schedule over one pass
 * of min(images, max_images_per_pass) images plus the feature rows of mvd_fid_update; never smaller for more images. */
int64_t mvd_fid_workspace_bytes(mvd_fid_t* v, int images);
int mvd_fid_bind_workspace(mvd_fid_t* v, void* ws, int64_t bytes);
/* images [n][3][h][w], dtype 0: uint8, 1: fp32 in [0, 1] (quantised as trunc(clamp(x, 0, 1) * 255)) -> feat_out [n][D] fp32.
 * Weights (-10 / -11) and every pass size that will run, the shorter last one included (-4), are checked before anything is
 * launched.  No allocation, no host synchronisation; everything on `stream`. */
int mvd_fid_features(mvd_fid_t* v, const void* images, int dtype, int n, int h, int w, float* feat_out, void* stream);
/* the same, then sum[D] += sum_i f_i and cov_sum[D][D] += sum_i f_i f_i^T in fp64 (mvd_op_feature_stats over all n rows at once) */
int mvd_fid_update(mvd_fid_t* v, const void* images, int dtype, int n, int h, int w, double* sum, double* cov_sum, void* stream);
/* The new operators one by one.  conv_relu_slice: x bf16 NHWC [batch][h][w][ld_in], channels [cin_off, cin_off + cin) ->
 * out[batch][oh][ow][ld_out], channels [c_off, c_off + cout) = max(conv + bias, 0), rounded once (bf16, or fp32 with out_f32);
 * nothing outside the slice is written.  (kh, kw) one of 1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1; stride 1 or 2; oh = (h + 2 pad_h -
 * kh) / stride + 1; taps outside the image are exact zeros.  w_packed as above.  Every channel count, offset and row stride is a
 * multiple of 16.  bf16 MFMA, fp32 accumulation over K = kh kw cin in (ky, kx, c) order, no split-K. */
int mvd_op_conv_relu_slice(const void* x, int batch, int h, int w, int ld_in, int cin_off, int cin, const void* w_packed, const float* bias, int kh, int kw,
                           int stride, int pad_h, int pad_w, int cout, void* out, int ld_out, int c_off, int out_f32, void* stream);
/* 3x3 pool of channels [cin_off, cin_off + c) of x bf16 NHWC into channels [c_off, c_off + c) of out.  mode 0: average, stride
 * 1, pad 1, over the in-image taps only (fp32 sum in tap order, a true division by their count, one rounding); 1: maximum,
 * stride 1, pad 1; 2: maximum, stride 2, no padding, floor.  Multiples of 8 channels. */
int mvd_op_pool3x3_slice(const void* x, int batch, int h, int w, int ld_in, int cin_off, int c, int mode, void* out, int ld_out, int c_off, void* stream);
/* the front end: src [batch][3][h][w] (dtype as above) -> out bf16 NHWC [batch][299][299][16], channels 3.. zero: TF1-legacy
 * bilinear resize (src = dst * float32(in / out), i0 = floor, i1 = min(i0 + 1, in - 1), top = tl + (tr - tl) wx, out = top +
 * (bot - top) wy, every operation rounded as written), then (v - 128) / 128 */
int mvd_op_resize_tf1(const void* src, int dtype, int batch, int h, int w, void* out, void* stream);
/* x fp32 [batch][pixels][c] -> out[batch][c] = (sum over the pixels in order) / pixels */
int mvd_op_global_mean(const float* x, int batch, int pixels, int c, float* out, void* stream);
/* f fp32 [n][d], d a multiple of 64: sum[d] += sum_i f_i, cov_sum[d][d] += sum_i f_i f_i^T, converted to fp64 first, on
 * v_mfma_f64_16x16x4_f64 with the images as K (zero padded to a multiple of 4), in image order; no atomics. */
int mvd_op_feature_stats(const float* f, int n, int d, double* sum, double* cov_sum, void* stream);

/* ---- KID and the Inception score on the same pool3 features ------------------------------------- */
/* Replaces: everything behind the network in torchmetrics' KernelInceptionDistance and InceptionScore(feature=
 * "logits_unbiased").  All five: int status with mvd_last_error, every argument checked on the host before anything is launched,
 * no allocation, no host synchronisation, everything on `stream`; no floating-point atomics, so two calls give the same bits.
 *
 * kid_mmd: f_real [n_real][d], f_fake [n_fake][d] fp32 (16-byte aligned, d a multiple of 64); idx int32 [subsets][2][m], slot 0
 * rows of f_real, slot 1 rows of f_fake (an index outside [0, n) is clamped, never dereferenced: validate on the host), 2 <= m <=
 * min(n_real, n_fake).  Per subset, with x / y the gathered rows in fp64 and k(a, b) = (a.b gamma + coef)^degree (the dot product
 * on v_mfma_f64_16x16x4_f64 over d in order, never split; the power by repeated multiplication, degree >= 1):
 *   S_xx = sum_{i != j} k(x_i, x_j), S_yy likewise, S_xy = sum_{i, j} k(x_i, y_j)   (i, j positions in the subset)
 *   out[s] = (S_xx + S_yy) / (m (m - 1)) - 2 S_xy / m^2     evaluated as written, IEEE division, no contraction
 * and sums[s] = {S_xx, S_yy, S_xy} when sums is not NULL.  64 x 64 tiles, one partial each in ws (xx and yy: the tiles on and above
 * the diagonal, those above counted twice), added in tile order.  No m x m matrix is written anywhere. */
int64_t mvd_op_kid_workspace_bytes(int subsets, int m);
int mvd_op_kid_mmd(const float* f_real, int n_real, const float* f_fake, int n_fake, int d, const int* idx, int subsets, int m, int degree, double gamma,
                   double coef, void* ws, int64_t ws_bytes, double* sums /* [subsets][3], may be NULL */, double* out /* [subsets] */, void* stream);
/* out[n][classes] = f[n][d] . w[classes][d]^T, all fp32, no bias (torch-fidelity's logits_unbiased: 1008 x 2048); d a multiple of
 * 4, f and w 16-byte aligned.  fp32 fma accumulation in an order that depends on d alone: a row's logits are the same bits alone
 * and inside any batch. */
int mvd_op_fc_logits(const float* f, int n, int d, const float* w, int classes, float* out, void* stream);
/* The Inception-score head in fp64 from fp32 logits [n][classes]; row j of the shuffled order is row perm[j] (int32 [n]).  Chunks
 * as torch.chunk(splits): ceil(n / splits) rows each, the last one shorter, possibly fewer than `splits` of them; their number
 * goes to *n_chunks_out (host, may be NULL).  Per row lse = max + log sum exp(x - max); per (chunk, class) mean_p = (sum over the
 * chunk's rows in row order of exp(x - lse)) / rows; per row kl = sum_c p ((x - lse) - log mean_p) in class order; out[chunk] =
 * exp(mean of kl over its rows in row order).  out holds at least min(splits, n) doubles. */
int64_t mvd_op_inception_score_workspace_bytes(int n, int classes, int splits);
int mvd_op_inception_score(const float* logits, int n, int classes, const int* perm, int splits, void* ws, int64_t ws_bytes, double* out,
                           int* n_chunks_out /* host */, void* stream);

/* ---- precision / recall and density / coverage on the same pool3 features ------------------------ */
/* Replaces: everything behind the network in torch-fidelity's `prc` metric (Kynkaanniemi et al. 2019) and in the `prdc`
 * package (Naeem et al. 2020).  All three: int status with mvd_last_error, every argument checked on the host before anything is
 * launched, no allocation, no host synchronisation, everything on `stream`; no floating-point atomics.
 *
 * Every comparison is on SQUARED distances, D2(a, b) = max(0, (|a|^2 + |b|^2) - 2 a.b) in fp64 from fp32 rows of d floats (d a
 * multiple of 64, 16-byte aligned): the dot product on v_mfma_f64_16x16x4_f64 over d in order, never split; the norms fp64 fma
 * chains in a fixed order.  No n x n matrix is written anywhere.
 *
 * knn_radii: radii_sq[i] = the (k + 1)-th smallest value of row i of D2(f, f), the row's own diagonal entry counted
 * (kthvalue(k + 1)); knn_sq, when not NULL, receives the row's k + 1 smallest values in ascending order, [n][k + 1] (so one pass
 * at k = 5 also serves k = 3).  1 <= k <= 15, n >= k + 1.  The columns are split into parts over a 2-D grid and a merge kernel
 * takes the k + 1 smallest of the parts' lists; force_parts 0 = automatic, otherwise the number of parts (at most one per 64
 * columns).  The k + 1 smallest values of a multiset do not depend on order: any force_parts and any two calls give the same bits.
 * ws holds the parts' lists. */
int64_t mvd_op_knn_radii_workspace_bytes(int n, int k, int force_parts);
int mvd_op_knn_radii(const float* f, int n, int d, int k, int force_parts, double* radii_sq /* [n] */, double* knn_sq_or_null /* [n][k + 1] */, void* ws,
                     int64_t ws_bytes, void* stream);
/* The predicate P[j][i] = D2(q_j, r_i) <= r_radii_sq[i] (closed = 1) or < (closed = 0), never stored: hits_per_query[j] = sum_i
 * P[j][i] and hits_per_ref[i] = sum_j P[j][i], int32, zeroed by the call, added with integer atomics (exact in any order).
 * Either output may be NULL.  With radii = knn_radii(r, k):
 *   precision = #{j : hits_per_query[j] > 0} / nq (q = fake, r = real, closed), recall the same with the sides exchanged;
 *   density = sum_j hits_per_query[j] / (k nq), coverage = #{i : hits_per_ref[i] > 0} / nr (q = fake, r = real, open). */
int mvd_op_manifold_counts(const float* q, int nq, const float* r, int nr, int d, const double* r_radii_sq, int closed, int32_t* hits_per_query,
                           int32_t* hits_per_ref, void* stream);

/* ---- image front end of the data loader (N13): composite on white, LANCZOS resize, normalisation ----------------------
 * What the reference's dataset does to every decoded render with PIL on the host (objaverse_dataset.py:279-294, :259-266):
 * Image.alpha_composite(white, img).convert("RGB") (channels == 4 only), resize((out_w, out_h), LANCZOS) -- Pillow's 8-bit
 * two-pass resample in integers, byte for byte -- and float(byte) / 127.5f - 1.0f (an fp32 division and an fp32 subtraction).
 * src [batch][h][w][channels] uint8 on the device (channels 3 or 4: the layout of np.array(Image.open(...))), any alignment;
 * when src is a multiple of 4 but not of 16, the 16-byte loads start at src rounded down to 16 bytes, i.e. up to 12 bytes in front
 * of the buffer are read (same 16-byte line, so never another page; the values are not used);
 * out_u8 [batch][out_h][out_w][3] uint8 and / or out_f32 [batch][3][out_h][out_w] fp32, at least one not NULL.  A pass whose
 * sizes are equal is skipped.  The workspace (256-byte aligned, workspace_bytes(...) bytes) holds the coefficient tables and the
 * uint8 intermediate; the tables are built once per geometry on the host and kept for the life of the process (tens of KB each; the
 * first 64 geometries also keep a page-locked copy for the upload, later ones upload from pageable memory).  Nothing synchronises.  Refused: a geometry whose
 * weights could overflow the 32-bit accumulator, and a horizontal scale above ~9 (the source span of one workgroup).
 * image_frontend_spans: {columns, rows} of a workgroup of the horizontal kernel, then of the vertical kernel (for tests that
 * plant values on both sides of every boundary). */
int mvd_op_image_frontend_spans(int* out4);
int64_t mvd_op_image_frontend_workspace_bytes(int batch, int h, int w, int channels, int out_h, int out_w);
int mvd_op_image_frontend(const uint8_t* src, int batch, int h, int w, int channels, int out_h, int out_w, uint8_t* out_u8, float* out_f32,
                          void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
