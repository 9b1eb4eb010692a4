/*
 * vitx.h -- C ABI of libvitx.so, the MI355X (gfx950) ViT forward/backward engine.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json: everything the
 * reference's Python classes hand to TensorFlow is handed to this library instead.
 * The reference exposes no FFI of its own (it is 24 files of Keras model definitions);
 * each entry point below cites the reference interface it replaces (paths relative to
 * /root/reference).  Plain C: pointers and sizes only, no C++/torch types, no exceptions.
 *
 * Conventions
 *   - every function returns int32 status: 0 = VITX_OK, <0 = error; the message of the last
 *     failure on the calling thread is available from vitx_last_error().
 *   - host buffers are borrowed for the duration of the call; the library owns all device memory
 *     (params, grads, saved activations, workspaces) unless arenas are bound with vitx_bind_arenas.
 *   - "_dev" variants take device pointers (inputs already resident in HBM) and are asynchronous
 *     on the handle's stream; the host-pointer variants synchronise before returning.
 *   - one handle <-> one GPU <-> one host thread at a time; different handles may be driven from
 *     different threads / processes (data parallel = one process per GPU, one handle each).
 *   - tensors are row-major fp32 at the boundary; images are NHWC like the reference's
 *     tf.random.normal([b, H, W, 3]) (vit_tensorflow/vit.py:193).
 */
#ifndef VITX_H_
#define VITX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VITX_OK 0
#define VITX_ERR_INVALID (-1)      /* bad argument / config (mirrors the reference's AssertionError sites) */
#define VITX_ERR_HIP (-2)          /* HIP runtime failure */
#define VITX_ERR_UNSUPPORTED (-3)  /* valid in the reference, not yet handled by the engine */
#define VITX_ERR_STATE (-4)        /* call order (e.g. backward without forward) */
#define VITX_ERR_COMM (-5)         /* RCCL failure */

enum { VITX_VARIANT_VIT = 0, VITX_VARIANT_DEEPVIT = 1, VITX_VARIANT_CAIT = 2, VITX_VARIANT_PATCH_MERGER = 3 };
enum { VITX_POOL_CLS = 0, VITX_POOL_MEAN = 1 };
/* FP32_PARITY: fp32 storage and fp32 FMA everywhere (gates "logits within 1e-3 of the reference").
 * BF16: bf16 GEMM/attention operands on MFMA, fp32 accumulation, statistics and residual stream.
 * BF16X3: the FP32_PARITY data path (fp32 storage, statistics, softmax, GELU, gradients) with every large GEMM evaluated as three bf16 MFMA
 *   products of operands split into bf16 hi + lo parts (~2^-16 per product): the 1e-3 gate at matrix-pipe speed. */
enum { VITX_COMPUTE_FP32_PARITY = 0, VITX_COMPUTE_BF16 = 1, VITX_COMPUTE_BF16X3 = 2 };

/* Mirrors the constructor kwargs 1:1:
 *   ViT(image_size, patch_size, num_classes, dim, depth, heads, mlp_dim, pool, dim_head, dropout,
 *       emb_dropout)                                   vit_tensorflow/vit.py:107-108
 *   DeepViT(... same ...)                              vit_tensorflow/deepvit.py:113-114
 *   CaiT(..., cls_depth, ..., layer_dropout)           vit_tensorflow/cait.py:156-157 */
typedef struct vitx_config {
  int32_t variant;
  int32_t image_h, image_w;   /* pair(image_size)  vit.py:133 */
  int32_t patch_h, patch_w;   /* pair(patch_size)  vit.py:134 */
  int32_t channels;           /* 3 (the reference's Rearrange infers it from the input) */
  int32_t num_classes, dim, depth, cls_depth, heads, dim_head, mlp_dim;
  int32_t pool;               /* vit.py:139 */
  float dropout, emb_dropout, layer_dropout;
  float ln_eps;               /* Keras LayerNormalization default 1e-3 */
  int32_t compute;
  int32_t max_batch;          /* device buffers are sized once for this batch */
  int32_t device_id;
  /* parallel_vit.ViT(..., num_parallel_branches=2) (parallel_vit.py:119-133): every layer is a sum of this many attention blocks
   * followed by a sum of this many feed-forward blocks, each with its own PreNorm (parallel_vit.py:36-42,104-117).  0 or 1 = the
   * ordinary ViT.  variant must be VITX_VARIANT_VIT. */
  int32_t num_parallel_branches;
  /* VITX_VARIANT_PATCH_MERGER = vit_with_patch_merger.ViT(..., patch_merge_layer=None, patch_merge_num_tokens=8)
   * (vit_with_patch_merger.py:136-183): no cls token, mean pooling, and after layer index
   * (patch_merge_layer > 0 ? patch_merge_layer : depth / 2) - 1 the tokens are merged to patch_merge_num_tokens by PatchMerger
   * (LayerNorm + learned-query attention pooling, vit_with_patch_merger.py:42-55,117,131-132). */
  int32_t patch_merge_layer, patch_merge_num_tokens;
  /* vit_for_small_dataset.ViT (vit_for_small_dataset.py:159-215): != 0 replaces the patch embedding by SPT -- the image concatenated with its four
   * one-pixel shifts, unfolded, LayerNorm, Dense (:142-157) -- and every attention by LSA: softmax scale exp(temperature) with a learned per-layer
   * scalar, diagonal of the scores masked (:88-121).  Needs variant VITX_VARIANT_VIT, num_parallel_branches <= 1 and patch_h == patch_w (the
   * reference's SPT hands patch_size to p1 and p2, :147); dim_head in {16, 32, 64} and at most 288 tokens, else VITX_ERR_UNSUPPORTED.
   * 0 (a zeroed struct) = off: the handle is exactly the ordinary one. */
  int32_t small_dataset;
  /* cct.TransformerEncoderLayer (cct.py:139-174): != 0 changes the data flow of every block to x1 = x + attn(ln1(x)), x2 = ln2(x1),
   * out = x2 + fc2(gelu(fc1(x2))) -- the second LayerNorm's result is the MLP input AND the residual stream -- and keeps to_out for heads == 1
   * (cct.py:117-122 always projects).  The parameter table is the ordinary ViT's.  Needs variant VITX_VARIANT_VIT, num_parallel_branches <= 1,
   * small_dataset == 0 and dropout == 0.  Such a handle serves vitx_cct_* through the device-pointer transformer entry; its image entry points
   * return VITX_ERR_UNSUPPORTED.  0 (a zeroed struct) = off: the handle is exactly the ordinary one. */
  int32_t cct_block;
  /* nest.Transformer (nest.py:77-148) run on (b * blocks^2) independent sequences: != 0 keeps to_out for heads == 1 with dim_head == dim
   * (nest.py:88-91 always projects) and runs the plain-softmax form of the small-head attention kernels (attn_lsa.hip without mask and
   * temperature) for dim_head in {16, 32} and at most 288 tokens; dim_head 64 keeps the fused kernels, everything else the materialised path.
   * The parameter table is the ordinary ViT's.  Needs variant VITX_VARIANT_VIT, num_parallel_branches <= 1, small_dataset == 0 and
   * cct_block == 0.  Such a handle serves vitx_nest_* through the device-pointer transformer entry; its image entry points return
   * VITX_ERR_UNSUPPORTED.  0 (a zeroed struct) = off: the handle is exactly the ordinary one.  Whether the small-head kernels run is the
   * composite's choice per handle (vitx_nest_config.small_attn). */
  int32_t nest_block;
  /* twins_svt.GlobalAttention (twins_svt.py:158-190) as the attention of every block: > 0 is the key / value reduction k.  The tokens of a
   * sequence are the image_h x image_w map (patch_h = patch_w = 1) in row-major order; to_q is a Dense on every token (:167,179), to_kv the
   * 'valid' Conv2D of kernel and stride k on the normalised map (:168,180), i.e. a Dense [k*k*dim, 2*inner] on the (image_h / k) x (image_w / k)
   * unfolded windows ((p1 p2 c) feature order = the Keras kernel's), then softmax(q k^T * dim_head^-0.5) v of image_h * image_w queries against
   * (image_h / k)(image_w / k) keys.  The block's table has attn.to_q.kernel [dim, inner] and attn.to_kv.kernel [k*k*dim, 2*inner] instead of
   * attn.to_qkv.kernel.  Needs nest_block != 0 (and so everything that flag needs) and image_h, image_w divisible by k; the transformer entry
   * takes exactly image_h * image_w tokens per sequence.  In the bf16 mode the attention of at most 64 keys at dim_head 64 runs the few-key kernels
   * (attn_fewkey.hip) unless VITX_GENERIC_ATTN is set or the composite switches them off.  0 (a zeroed struct) = off: the handle is exactly as before. */
  int32_t global_k;
  /* cvt.Attention (cvt.py:94-127) as the attention of every block -- the last spare word of the struct, as two halves: conv_proj_kernel > 0 is
   * proj_kernel, conv_proj_stride kv_proj_stride (>= 1).  The tokens of a sequence are the image_h x image_w map (patch_h = patch_w = 1) in
   * row-major order.  to_q and to_kv are DepthWiseConv2d (:79-92): a depthwise 'SAME' convolution without bias (stride 1 for q,
   * conv_proj_stride for kv: ceil(image_h / s) x ceil(image_w / s) keys, TensorFlow's uneven padding), BatchNormalization (eps bn_eps of the
   * composite, 1e-5) over every position of the call's batch, and a pointwise Dense without bias (csrc/cvt_ops.hip).  The block's table has
   * attn.to_q.dw.kernel [k, k, 1, dim], attn.to_q.bn.gamma / .beta / .moving_mean / .moving_variance [dim], attn.to_q.pw.kernel [dim, inner]
   * and the same under attn.to_kv (pw.kernel [dim, 2 * inner]) instead of attn.to_qkv.kernel.  Needs nest_block != 0 and global_k == 0; the
   * transformer entry takes exactly image_h * image_w tokens per sequence.  In the bf16 mode the attention of at most 64 keys at dim_head 64
   * runs the few-key kernels unless VITX_GENERIC_ATTN is set or the composite switches them off.  The moving statistics are read only by
   * forwards the composite marks as inference (vitx_cvt_forward, training == 0); no forward updates them and their gradients are zeros.
   * 0 (a zeroed struct) = off: the handle is exactly as before.  The struct has no spare word left. */
  int16_t conv_proj_kernel, conv_proj_stride;
} vitx_config;

typedef struct vitx_engine* vitx_handle;

/* per-kernel-class timing collected between vitx_profile_begin/_end (HIP events on the handle's stream) */
typedef struct vitx_kernel_stat {
  char name[48];
  int64_t launches;
  double total_ms;
  double flops;   /* algorithmic FLOPs issued by these launches */
  double bytes;   /* algorithmic HBM bytes (compulsory reads + writes) */
} vitx_kernel_stat;

/* called from vitx_backward* on the host as soon as every kernel producing grads[offset, offset+count)
 * has been enqueued on the handle's stream (gradient buckets for overlapped all-reduce) */
typedef void (*vitx_grad_ready_fn)(void* user, int64_t offset_elems, int64_t count_elems);

const char* vitx_version(void);
const char* vitx_last_error(void);

/* ---- parameter table (host only, no GPU needed).  Replaces Keras' model.weights / get_weights()
 * ordering (inherited from tf.keras.Model, used by mae.py:36-38).  Order is explicit and documented
 * in DESIGN.md; layouts are Keras': Dense kernel [in,out], bias [out], LN gamma/beta [d]. */
int32_t vitx_param_table_size(const vitx_config* cfg, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_param_table_entry(const vitx_config* cfg, int64_t index, char* name, int32_t name_cap,
                               int64_t shape[4], int32_t* rank, int64_t* offset_elems);

/* ---- lifetime: ViT.__init__ (vit.py:107-157), DeepViT.__init__ (deepvit.py:113-137),
 * CaiT.__init__ (cait.py:156-178).  Validation errors carry the reference's assertion text. */
int32_t vitx_create(const vitx_config* cfg, vitx_handle* out);
int32_t vitx_destroy(vitx_handle h);
int32_t vitx_get_config(vitx_handle h, vitx_config* out);   /* the (defaulted) config a handle was built with */

/* ---- weights: Keras set_weights/get_weights (flat fp32 blob in table order) */
int32_t vitx_set_params(vitx_handle h, const float* host_blob, int64_t n_elems);
int32_t vitx_get_params(vitx_handle h, float* host_blob, int64_t n_elems);
int32_t vitx_get_grads(vitx_handle h, float* host_blob, int64_t n_elems);
/* device arenas (fp32, table order) -- for optimizers / collectives living outside the library */
int32_t vitx_params_dev(vitx_handle h, float** dev_ptr, int64_t* n_elems);
int32_t vitx_grads_dev(vitx_handle h, float** dev_ptr, int64_t* n_elems);
/* use caller-owned device arenas (e.g. torch tensors) instead of the library's; either may be NULL */
int32_t vitx_bind_arenas(vitx_handle h, float* params_dev, float* grads_dev);
/* tell the engine the fp32 params changed on device (re-derives the bf16 operand copies) */
int32_t vitx_params_changed(vitx_handle h);

/* ---- forward: ViT.call / DeepViT.call / CaiT.call (vit.py:159-177, deepvit.py:139-157,
 * cait.py:180-194).  img NHWC fp32 [b,H,W,C]; H,W may be smaller than the configured image as long
 * as they divide by the patch (pos_embedding is sliced, vit.py:165).  logits [b,num_classes]. */
int32_t vitx_forward(vitx_handle h, const float* img_host, int32_t b, int32_t H, int32_t W,
                     int32_t training, uint64_t seed, float* logits_host);
int32_t vitx_forward_dev(vitx_handle h, const float* img_dev, int32_t b, int32_t H, int32_t W,
                         int32_t training, uint64_t seed, float* logits_dev);

/* ---- backward: the VJP TensorFlow's GradientTape would compute for the forward above
 * (README.md:746-749 is the reference's only mention).  Requires a preceding forward with the same
 * b; fills the gradient arena (overwrites, no accumulation).  dimg may be NULL (TF does not
 * differentiate w.r.t. an un-watched image). */
int32_t vitx_backward(vitx_handle h, const float* dlogits_host, float* dimg_host_or_null);
/* Long sequences: Attention.call (vit.py:73-82) past the 288 tokens the fused bf16 attention kernels hold in LDS, e.g. ViT-B/16 at 384 px (577
 * tokens).  on != 0: such a sequence runs the streamed-key kernels (csrc/attn_stream.hip: K / V chunks through an LDS ring, online softmax, the
 * [b, heads, n, n] scores never in HBM, no score workspace) instead of the materialised path; at n <= 288, or under VITX_GENERIC_ATTN, nothing
 * changes.  0 (the default of every new handle) = as before.  vitx_config has no spare word, hence a setter.  Call it between steps, at any time:
 * after a forward with training == 0 (a step of its own: a forward-only caller may switch whenever it likes) and after any backward.  Between a
 * forward with training != 0 and its backward it returns VITX_ERR_STATE.  A backward always takes the path its forward took.  Whatever
 * `on` is, a handle that can never take the path -- FP32_PARITY or BF16X3 compute, a variant other than VITX_VARIANT_VIT, dim_head != 64,
 * small_dataset / cct_block / nest_block -- returns VITX_ERR_UNSUPPORTED with the reason in vitx_last_error().  Sequence bounds: b * heads <= 65535
 * and n * 3 * heads * 64 < 2^30 elements per image, else the forward returns VITX_ERR_UNSUPPORTED. */
int32_t vitx_set_long_attn(vitx_handle h, int32_t on);
/* Forward from caller-supplied patch rows [b, np, patch_dim] (fp32) in place of the image + Rearrange: the first layer(s) of T2T-ViT's
 * patch_embedding are a tokenizer pipeline (t2t.py:59-77) whose output feeds the same Dense, cls / position rows, transformer and head
 * (t2t.py:99-121).  A backward after it returns d(patches) [b, np, patch_dim] through the dimg argument. */
/* One shot: the NEXT host-pointer forward entry on this handle (vitx_forward, vitx_forward_distill, or vitx_distill_forward of a
 * wrapper around it) reads its image argument as patch rows [b, np, patch_dim]; H / W are ignored there.  np = 0 clears it. */
int32_t vitx_set_patch_input(vitx_handle h, int32_t np);
int32_t vitx_forward_patches(vitx_handle h, const float* patches_host, int32_t b, int32_t np, int32_t training, uint64_t seed,
                             float* logits_host);
int32_t vitx_forward_patches_dev(vitx_handle h, const float* patches_dev, int32_t b, int32_t np, int32_t training, uint64_t seed,
                                 float* logits_dev_or_null);
int32_t vitx_backward_dev(vitx_handle h, const float* dlogits_dev, float* dimg_dev_or_null);

/* ---- encoder.transformer(tokens, training=training) on arbitrary [b,n,dim] tokens (mae.py:69, simmim.py:116,
 * efficient.py:47, mpp.py:212).  ViT / DeepViT only.  training != 0 applies the model's Dropout layers (vit.py:41,43,64) with
 * masks drawn from `seed`, as vitx_forward does; the VJP below replays them. */
int32_t vitx_transformer_forward(vitx_handle h, const float* tokens_host, int32_t b, int32_t n,
                                 int32_t training, uint64_t seed, float* out_host);
/* VJP of the call above (what GradientTape gives the wrappers that train through encoder.transformer: mae.py:69 + README.md:746-749):
 * d(out) [b,n,dim] -> d(tokens) [b,n,dim] (may be NULL); the gradient arena holds the transformer's parameter gradients, every
 * other entry is zero.  Requires a preceding vitx_transformer_forward (same handle, no full forward in between). */
int32_t vitx_transformer_backward(vitx_handle h, const float* dout_host, float* dtokens_host_or_null);

/* ---- stand-alone patch unfold: Rearrange('b (h p1) (w p2) c -> b (h w) (p1 p2 c)') (vit.py:142,
 * deepvit.py:122, cait.py:164).  Pure index arithmetic: bit-exact. */
int32_t vitx_patch_unfold(const float* img_host, int32_t b, int32_t H, int32_t W, int32_t C,
                          int32_t ph, int32_t pw, float* out_host);

/* ---- efficient.ViT(image_size, patch_size, num_classes, dim, transformer, pool='cls') (efficient.py:12-56): the model is a shell
 * around a transformer object supplied by the caller.  On a ViT handle (normally built with depth = 0; the block parameters of a
 * deeper handle are simply not used) the four entry points below are that shell and its VJP:
 *   embed_forward   patch_embedding + cls token + pos_embedding[:, :n+1] (efficient.py:40-46): img NHWC -> tokens [b, np+1, dim]
 *   head_forward    pooling + mlp_head (efficient.py:49-54): x [b, n, dim] (whatever the transformer returned) -> logits
 *   head_backward   d(logits) -> d(x) [b, n, dim]; fills the mlp_head.* entries of the gradient arena
 *   embed_backward  d(tokens) [b, np+1, dim] -> fills pos_embedding (rows beyond np+1 zero), cls_token, patch_embedding.*;
 *                   optional d(img)
 * Validation error text follows efficient.py:18.  The _dev forms take device pointers and stay asynchronous on the handle's
 * stream (dlogits_dev NULL = the engine's internal dlogits); tokens / x are contiguous fp32. */
int32_t vitx_embed_forward(vitx_handle h, const float* img_host, int32_t b, int32_t H, int32_t W, float* tokens_host);
int32_t vitx_embed_forward_dev(vitx_handle h, const float* img_dev, int32_t b, int32_t H, int32_t W, float* tokens_dev);
int32_t vitx_head_forward(vitx_handle h, const float* x_host, int32_t b, int32_t n, float* logits_host);
int32_t vitx_head_forward_dev(vitx_handle h, const float* x_dev, int32_t b, int32_t n, float* logits_dev_or_null);
int32_t vitx_head_backward(vitx_handle h, const float* dlogits_host, float* dx_host);
int32_t vitx_head_backward_dev(vitx_handle h, const float* dlogits_dev_or_null, float* dx_dev);
int32_t vitx_embed_backward(vitx_handle h, const float* dtokens_host, float* dimg_host_or_null);
int32_t vitx_embed_backward_dev(vitx_handle h, const float* dtokens_dev, float* dimg_dev_or_null);

/* ---- SPT(dim, patch_size)(img) on its own (vit_for_small_dataset.py:142-157) on a small_dataset handle: Dense(LN(unfold(concat(x, shifts)))),
 * [b, np, dim]; no cls token, no position rows.  Forward only. */
int32_t vitx_spt_forward(vitx_handle h, const float* img_host, int32_t b, int32_t H, int32_t W, float* tokens_host);
int32_t vitx_spt_forward_dev(vitx_handle h, const float* img_dev, int32_t b, int32_t H, int32_t W, float* tokens_dev);

/* ---- encoder.patch_embedding.layers[1] on its own: the nn.Dense(units=dim) of vit.py:143 as the wrappers borrow it (mae.py:37,52;
 * simmim.py:79,92; mpp.py:200) -- rows of unfolded patches [rows, p1*p2*C] -> [rows, dim]; no cls token, no position embedding.
 * Forward only (the trainable wrappers are vitx_mim_* / vitx_distill_*). */
int32_t vitx_patch_dense_forward(vitx_handle h, const float* patches_host, int32_t rows, float* out_host);

/* ---- T2T tokenizer: tf.image.extract_patches(x, sizes=[1,k,k,1], strides=[1,s,s,1], rates=[1,1,1,1], padding='SAME')
 * (RearrangeUnfoldTransformer.call, t2t.py:39-47) on NHWC x [b,H,W,C] -> [b, ceil(H/s), ceil(W/s), k*k*C], feature order
 * (ki, kj, c), TensorFlow's SAME rule (pad_total = max((out-1)*s + k - in, 0), pad_before = pad_total / 2, zeros outside).
 * Pure index arithmetic: bit-exact.  _backward is its VJP (overlapping windows summed in a fixed order).  Handle-free; the _dev
 * forms enqueue on `hip_stream` (NULL = the default stream). */
int32_t vitx_extract_patches_shape(int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, int32_t* oh, int32_t* ow, int32_t* feat);
int32_t vitx_extract_patches(const float* x_host, int32_t b, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, float* out_host);
int32_t vitx_extract_patches_backward(const float* dout_host, int32_t b, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride,
                                      float* dx_host);
int32_t vitx_extract_patches_dev(const float* x_dev, int32_t b, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride, float* out_dev,
                                 void* hip_stream);
int32_t vitx_extract_patches_backward_dev(const float* dout_dev, int32_t b, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride,
                                          float* dx_dev, void* hip_stream);

/* ---- loss gradient on device: d/dlogits of mean softmax cross-entropy
 * (tf.keras.losses.categorical_crossentropy(from_logits=True), distill.py:119).  Writes the
 * engine's internal dlogits (used by vitx_backward_dev(h, NULL, ...)) and optionally the mean loss. */
int32_t vitx_ce_loss_grad_dev(vitx_handle h, const int32_t* labels_dev, float inv_global_batch,
                              float* loss_dev_or_null);

/* ---- optimizer step on the device arenas ("next" row f1 of SURVEY.md section 8: the reference has no optimizer or trainer at
 * all; this turns forward+backward into a training step).  Uses the gradients of the last backward (all-reduced or not). */
int32_t vitx_adamw_step(vitx_handle h, float lr, float beta1, float beta2, float eps, float weight_decay);
int32_t vitx_sgd_step(vitx_handle h, float lr, float momentum, float weight_decay);

/* Optimizer state of a handle (AdamW first / second moments, SGD momentum: fp32 in the packed host order of vitx_get_params; the
 * AdamW step count).  A handle owns this state, so a caller that rebuilds its handle (a larger max_batch) carries it across with
 * this pair; have_m / have_v report which buffers exist, NULL host pointers skip the copy. */
int32_t vitx_get_opt_state(vitx_handle h, float* m_host_or_null, float* v_host_or_null, int64_t n_elems, int64_t* step,
                           int32_t* have_m, int32_t* have_v);
int32_t vitx_set_opt_state(vitx_handle h, const float* m_host_or_null, const float* v_host_or_null, int64_t n_elems, int64_t step);

/* ---- streams / sync */
int32_t vitx_set_stream(vitx_handle h, void* hip_stream); /* NULL = the handle's own stream */
int32_t vitx_sync(vitx_handle h);

/* ---- HIP graphs (no reference counterpart: replaces ~300 launches of a step by one when the step is launch-bound, e.g. the
 * README's batch-1 example).  Everything enqueued on the handle through the *_dev entry points between begin and end is recorded
 * instead of run; the captured device pointers (images, labels, logits) are baked in.  Run one eager step of the same geometry
 * first (first-use allocations and the GEMM variant measurements cannot be captured). */
int32_t vitx_graph_capture_begin(vitx_handle h);
int32_t vitx_graph_capture_end(vitx_handle h, void** graph_exec_out);
int32_t vitx_graph_launch(vitx_handle h, void* graph_exec);
int32_t vitx_graph_destroy(void* graph_exec);

/* ---- data parallel (no reference counterpart: batch-sharded replicas, mean-reduced gradients) */
int32_t vitx_set_grad_ready_callback(vitx_handle h, vitx_grad_ready_fn fn, void* user);
int32_t vitx_comm_unique_id(void* out_128_bytes);
int32_t vitx_comm_init(vitx_handle h, int32_t rank, int32_t world, const void* unique_id_128_bytes);
/* Overlapped exchange (SURVEY.md 8(e), Appendix B "grads live in one contiguous arena ... buckets are contiguous slices; side stream + events"):
 * enable != 0 -> from the next backward on, every bucket of the gradient arena is all-reduced (and scaled by 1/world) on the handle's own
 * communication stream the moment the backward pass has enqueued its last producer; vitx_allreduce_grads then only sends what is left and orders the
 * compute stream behind the last bucket.  bucket_bytes: fp32 bytes per bucket (0 = 32 MiB); wire_bf16 != 0: the collective moves bf16 copies
 * (half the xGMI bytes; each rank's addend is rounded once).  Call after vitx_comm_init, between steps. */
int32_t vitx_comm_overlap(vitx_handle h, int32_t enable, int64_t bucket_bytes, int32_t wire_bf16);
/* out4 = {buckets, buckets the last exchange sent from inside the backward pass, elements per bucket, Dense launches that found a collective in flight} */
int32_t vitx_comm_stats(vitx_handle h, int64_t* out4);
/* leave the group: the communicator, the communication stream and the wire buffer are released and the handle is single-rank again (a later
 * vitx_comm_init may join another group).  Call between steps -- an exchange in progress is joined first. */
int32_t vitx_comm_destroy(vitx_handle h);
int32_t vitx_allreduce_grads(vitx_handle h); /* RCCL mean over ranks of the gradient arena (bucketed; finishes an overlapped exchange) */

/* ---- measurement / debugging */
/* Every VITX_* environment variable the library reads, one line per switch: "NAME<TAB>class<TAB>state<TAB>what it does\n" with class in
 * {tuning (same results), path (another validated code path; results within the same oracle gates), diag (timing experiment: may corrupt
 * results)} and state in {unset, set=<value>, ignored (a diag switch in a release build)}.  A release library ignores the diag class; only
 * lib/libvitx_diag.so (build.py --diag) honours it.  Writes at most cap bytes (NUL-terminated); *needed = bytes of the full text + 1. */
int32_t vitx_debug_switches(char* out, int64_t cap, int64_t* needed);
int32_t vitx_profile_begin(vitx_handle h);
int32_t vitx_profile_end(vitx_handle h, vitx_kernel_stat* out, int32_t cap, int32_t* n_out);
int32_t vitx_workspace_bytes(vitx_handle h, int64_t* bytes);
/* copy a saved activation of the last forward to the host as fp32 (bisecting parity failures, per-stage parity tests);
 * `which` in {"embed","x_in","y1","qkv","attn_out","x_mid","y2","hpre","act","x_out","pooled"}; after vitx_transformer_forward the
 * block names describe that call's [b, n] rows.  In the bf16 mode "hpre" holds gelu'(h), what the backward multiplies by.
 * LayerNorm statistics "mean1","rstd1","mean2","rstd2" [rows] and the softmax log-sum-exp "lse" [b, heads, n] (fused and streamed-key
 * attention only) are fp32.
 * Between a backward and the next forward, for the block whose backward ran last (`layer` must name it; layer 0 after a whole backward):
 *   "d_hpre" [rows, mlp_dim], "d_attn_out" [rows, inner] (blocks with a to_out Dense), "d_qkv" packed [rows, 3 inner],
 *   "d_y1" [rows, dim] -- the buffer both input-gradient GEMMs of a block write: after a whole block backward it holds d(y1), not d(y2).
 * A variant or form that keeps one of these in another layout (CaiT [dq | dkv], reduced keys, the class-row last block) answers
 * "activation not available for this variant". */
int32_t vitx_debug_read(vitx_handle h, const char* which, int32_t layer, float* out_host,
                        int64_t cap_elems, int64_t* n_elems);
/* raw GEMM micro-benchmark on the handle's stream: C[M,N] = A[M,K] * B[N,K]^T (bf16 operands,
 * random data), returns the average ms over `iters` launches; `kernel` selects the tile variant */
int32_t vitx_bench_gemm(vitx_handle h, int32_t M, int32_t N, int32_t K, int32_t kernel,
                        int32_t epilogue, int32_t iters, float* avg_ms, float* max_abs_err);
/* full-size self-check of the bf16 MFMA GEMM launches, compared on the device with the k-ordered fp32-FMA kernel on the same bf16 operands
 * (test hook; the Dense layers of vit.py:39,42,59,63 at the benchmarked row count).  kind 0: C[M,N] = A[M,K] B[N,K]^T with fused epilogue
 * `epilogue` (codes of vitx_bench_gemm) on tile variant `kernel`; kind 1: the weight-gradient form dW[M=in, N=out] over K token rows with the
 * engine's split-K rule and slice reduction.  errs2[0] = max |got - want| / (1 + |want|); errs2[1] = the same for the second output
 * (epilogue 2) / the fused column sums (epilogue 4), the number of K slices (kind 1), else -1. */
int32_t vitx_check_gemm(vitx_handle h, int32_t kind, int32_t M, int32_t N, int32_t K, int32_t kernel,
                        int32_t epilogue, float* errs2);

/* ---- masked-image-modelling wrappers around a built encoder ("next" row f2 of SURVEY.md section 8):
 *   MAE(image_size, encoder, decoder_dim, masking_ratio, decoder_depth, decoder_heads, decoder_dim_head)   mae.py:17-45
 *   SimMIM(image_size, encoder, masking_ratio)                                                            simmim.py:68-84
 * The wrapper borrows the encoder handle (to_patch / patch_to_emb / pos_embedding[:, 1:] / .transformer: mae.py:36-38,
 * simmim.py:79-81) and owns its own parameters: MAE {enc_to_dec.kernel/.bias (only when encoder dim != decoder_dim, else the
 * reference's Identity), mask_token, decoder_pos_emb.embeddings, to_pixels.kernel/.bias} plus a decoder Transformer that is an
 * ordinary handle (vitx_mim_decoder: use its "transformer.*" table entries); SimMIM {mask_token, to_pixels.kernel/.bias}.
 * The random masking indices are an input (the reference draws them with tf.random.uniform + argsort / top_k, mae.py:58,
 * simmim.py:108): MAE int32 [b, num_patches] = rand_indices, whose first num_masked columns are the masked patches;
 * SimMIM int32 [b, num_masked] = masked_indices.  num_masked = int(masking_ratio * num_patches). */
/* MPP(image_size, transformer, patch_size, output_channel_bits, channels, max_pixel_val, mask_prob, replace_prob, random_patch_prob,
 *     mean, std)                                                                                              mpp.py:133-218
 * Masked patch prediction: the encoder's own embedding (patch Dense + cls + pos + dropout, mpp.py:200-209), its transformer on all
 * tokens (:212), a Dense to 2^(bits * channels) classes (`to_bits`, :149,213) and a loss over the masked positions (MPPLoss, :90-131).
 * Parameters {to_bits.kernel/.bias, mask_token}.  indices: int32 [b, num_masked] = the top_k draw of get_mask_subset_with_prob (:79-88),
 * num_masked = ceil(mask_prob * num_patches).  Two places where the reference's code does not do what it evidently means are reproduced
 * literally by default (literal_loss = 1) and documented in DESIGN.md: the in-place replacements of mpp.py:185,190 are written into
 * `.numpy()` COPIES and never reach the tensor (the transformer sees the unmasked patches; mask_token receives no gradient), and
 * MPPLoss passes (predictions, labels) to tf.nn.softmax_cross_entropy_with_logits(labels, logits) in swapped order with
 * clip_by_value(target, max_pixel_val, max_pixel_val), so the loss as written is log(2^(bits c)) * mean_i sum_j logits_ij.
 * literal_loss = 0: softmax cross-entropy of the masked positions' logits against the discretised mean colour of their patches. */
enum { VITX_MIM_MAE = 0, VITX_MIM_SIMMIM = 1, VITX_MIM_MPP = 2 };
typedef struct vitx_mim_config {
  int32_t kind;
  int32_t decoder_dim, decoder_depth, decoder_heads, decoder_dim_head; /* MAE only (mae.py:21-25) */
  /* MAE: 1 = the loss exactly as written, tf.reduce_mean(tf.square(pred_pixel_values, masked_patches)) (mae.py:90), where the
   * second positional argument of tf.square is `name`, i.e. mean(pred^2); 0 = the evidently intended mean((pred - masked_patches)^2).
   * SimMIM ignores it (simmim.py:128 is a plain L1). */
  int32_t literal_loss;
  double masking_ratio;            /* MPP: mask_prob */
  int32_t output_channel_bits;     /* MPP (mpp.py:137), default 3 */
  float max_pixel_val;             /* MPP (mpp.py:139), default 1.0 */
  int32_t has_norm;                /* MPP: 1 = un-normalise the target with norm_mean / norm_std (mpp.py:108-109), channels <= 4 */
  float norm_mean[4], norm_std[4];
  int32_t reserved[5];
} vitx_mim_config;
typedef struct vitx_mim* vitx_mim_handle;

int32_t vitx_mim_create(vitx_handle encoder, const vitx_mim_config* cfg, vitx_mim_handle* out);
int32_t vitx_mim_destroy(vitx_mim_handle m);           /* does not destroy the encoder */
vitx_handle vitx_mim_decoder(vitx_mim_handle m);       /* MAE: Transformer(dim=decoder_dim, ..., mlp_dim=4*decoder_dim) mae.py:43; else NULL */
int32_t vitx_mim_param_table_size(vitx_mim_handle m, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_mim_param_table_entry(vitx_mim_handle m, int64_t index, char* name, int32_t name_cap,
                                   int64_t shape[4], int32_t* rank, int64_t* offset_elems);
int32_t vitx_mim_set_params(vitx_mim_handle m, const float* host_blob, int64_t n_elems);
int32_t vitx_mim_get_params(vitx_mim_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_mim_get_grads(vitx_mim_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_mim_params_dev(vitx_mim_handle m, float** params_dev, float** grads_dev, int64_t* n_arena_elems);
int32_t vitx_mim_params_changed(vitx_mim_handle m);   /* the wrapper's fp32 params changed on device (like vitx_params_changed) */
int32_t vitx_mim_num_masked(vitx_mim_handle m, int32_t H, int32_t W, int32_t* num_patches, int32_t* num_masked);
/* MAE.call (mae.py:47-92) / SimMIM.call (simmim.py:86-130): returns the reconstruction loss.  The host variant validates the
 * indices (range, distinct per image: simmim.py:31) and synchronises; the _dev variant trusts them and stays asynchronous. */
int32_t vitx_mim_forward(vitx_mim_handle m, const float* img_host, int32_t b, int32_t H, int32_t W,
                         const int32_t* indices_host, int32_t training, uint64_t seed, float* loss_host);
int32_t vitx_mim_forward_dev(vitx_mim_handle m, const float* img_dev, int32_t b, int32_t H, int32_t W,
                             const int32_t* indices_dev, int32_t training, uint64_t seed, float* loss_dev_or_null);
/* VJP of the forward above for d(loss) = 1 (README.md:746-749 style training): wrapper gradients -> vitx_mim_get_grads,
 * encoder gradients -> the encoder's arena (transformer blocks, patch_embedding.*, pos_embedding rows 1..num_patches; all other
 * entries zero), decoder gradients -> the decoder handle's arena.  Unlike the reference -- whose `.numpy()` indexing
 * (mae.py:62, simmim.py:119) silently detaches everything upstream of it from the tape -- the gather is differentiable. */
int32_t vitx_mim_backward(vitx_mim_handle m);
/* copy a tensor of the last forward to the host: "pred", "target", "patches", "encoded", "decoded" (MAE) */
int32_t vitx_mim_read(vitx_mim_handle m, const char* which, float* out_host, int64_t cap_elems, int64_t* n_elems);

/* ---- knowledge distillation ("next" row f3 of SURVEY.md section 8).
 * DistillableViT.call(img, distill_token) (DistillMixin, distill.py:16-44): the token [dim] is appended after the position
 * embedding, attended with the other tokens, split off before pooling; returns logits [b,num_classes] and the per-image
 * distillation tokens [b,dim].  backward: cotangents of both outputs -> gradient arena, d(token) [dim], optional d(img).
 * Works on any ViT / DeepViT handle (DistillableViT adds no parameters of its own, distill.py:46-57). */
int32_t vitx_forward_distill(vitx_handle h, const float* img_host, int32_t b, int32_t H, int32_t W, int32_t training, uint64_t seed,
                             const float* distill_token_host, float* logits_host, float* distill_tokens_host);
int32_t vitx_backward_distill(vitx_handle h, const float* dlogits_host, const float* d_distill_tokens_host_or_null,
                              float* d_distill_token_host_or_null, float* dimg_host_or_null);

/* DistillWrapper(teacher, student, temperature, alpha, hard) (distill.py:87-134).  The teacher is any model: its logits are an
 * input (tf.stop_gradient, distill.py:114).  Own parameters: distillation_token [1,1,dim], distill_mlp.norm.{gamma,beta},
 * distill_mlp.{kernel,bias} (distill.py:101-106).  loss [b] = CE(labels, student_logits) * (1 - alpha) + distill_loss * alpha,
 * with labels [b,num_classes] one-hot or soft (categorical_crossentropy(from_logits=True), distill.py:119). */
typedef struct vitx_distill_config {
  float temperature, alpha; /* distill.py:88 defaults 1.0, 0.5 */
  int32_t hard;             /* 0: temperature-scaled KL to the teacher's softmax (distill.py:121-129); 1: cross-entropy against
                             * the teacher's argmax (distill.py:130-132: as written it passes rank-1 integer labels to
                             * categorical_crossentropy, which TensorFlow rejects; the engine computes the sparse form) */
  /* soft mode, 1 = exactly as written: keras.losses.KLDivergence is handed LOG-probabilities as y_pred (distill.py:122-124) and
   * clips them to [1e-7, 1], so the term is sum(y log(y / 1e-7)), constant in the student (zero gradient);
   * 0 = the evident intent KL(softmax(teacher / T) || softmax(distill_logits / T)) */
  int32_t literal_loss;
  int32_t reserved[8];
} vitx_distill_config;
typedef struct vitx_distill* vitx_distill_handle;

int32_t vitx_distill_create(vitx_handle student, const vitx_distill_config* cfg, vitx_distill_handle* out);
int32_t vitx_distill_destroy(vitx_distill_handle m);   /* does not destroy the student */
int32_t vitx_distill_param_table_size(vitx_distill_handle m, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_distill_param_table_entry(vitx_distill_handle m, int64_t index, char* name, int32_t name_cap,
                                       int64_t shape[4], int32_t* rank, int64_t* offset_elems);
int32_t vitx_distill_set_params(vitx_distill_handle m, const float* host_blob, int64_t n_elems);
int32_t vitx_distill_get_params(vitx_distill_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_distill_get_grads(vitx_distill_handle m, float* host_blob, int64_t n_elems);
/* DistillWrapper.call((img, labels), temperature, alpha, training) (distill.py:107-134); temperature <= 0 / alpha < 0 take the
 * constructor's values (distill.py:110-111).  loss: [b]. */
int32_t vitx_distill_forward(vitx_distill_handle m, const float* img_host, const float* labels_host, const float* teacher_logits_host,
                             int32_t b, int32_t H, int32_t W, int32_t training, uint64_t seed, float temperature, float alpha,
                             float* loss_host);
int32_t vitx_distill_forward_dev(vitx_distill_handle m, const float* img_dev, const float* labels_dev, const float* teacher_logits_dev,
                                 int32_t b, int32_t H, int32_t W, int32_t training, uint64_t seed, float temperature, float alpha,
                                 float* loss_dev_or_null);
/* VJP for the cotangent dloss [b] (NULL = ones: tape.gradient of a non-scalar target differentiates its sum): wrapper gradients
 * -> vitx_distill_get_grads, student gradients -> the student's arena. */
int32_t vitx_distill_backward(vitx_distill_handle m, const float* dloss_host_or_null);
/* the same, also returning d(loss)/d(input) of the student's forward: d(img) [b,H,W,C], or d(patches) [b,np,patch_dim] when that forward
 * took patch rows (vitx_set_patch_input: a T2T-ViT student, whose tokenizer in front of the handle continues the chain) */
int32_t vitx_distill_backward_input(vitx_distill_handle m, const float* dloss_host_or_null, float* dinput_host);
/* "student_logits", "distill_logits" [b,num_classes], "distill_tokens" [b,dim] of the last forward */
int32_t vitx_distill_read(vitx_distill_handle m, const char* which, float* out_host, int64_t cap_elems, int64_t* n_elems);

/* ---- CrossViT (cross_vit.py:232-301): two ImageEmbedders, `depth` x [sm Transformer, lg Transformer, CrossTransformer], two summed
 * mlp_heads.  A handle of its own (not a vitx_handle): parameter order in DESIGN.md section 7.  No data parallel, graph capture or
 * in-library optimizer step: the device arenas are exposed for optimizers outside the library. */
typedef struct vitx_crossvit_config {
  int32_t image_size, num_classes, sm_dim, lg_dim;
  int32_t sm_patch_size, sm_enc_depth, sm_enc_heads, sm_enc_mlp_dim, sm_enc_dim_head;
  int32_t lg_patch_size, lg_enc_depth, lg_enc_heads, lg_enc_mlp_dim, lg_enc_dim_head;
  int32_t cross_attn_depth, cross_attn_heads, cross_attn_dim_head, depth;
  float dropout, emb_dropout;   /* cross_vit.py:252-253 */
  float ln_eps;                 /* <= 0: Keras LayerNormalization default 1e-3 */
  int32_t compute;              /* VITX_COMPUTE_*: the encoders' mode; the cross layers run in fp32 in every mode */
  int32_t max_batch;
  int32_t device_id;
  int32_t reserved[8];
} vitx_crossvit_config;
typedef struct vitx_crossvit* vitx_crossvit_handle;
/* host only, no GPU needed; errors carry the reference's assertion text */
int32_t vitx_crossvit_param_table_size(const vitx_crossvit_config* cfg, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_crossvit_param_table_entry(const vitx_crossvit_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4],
                                        int32_t* rank, int64_t* offset_elems);
int32_t vitx_crossvit_create(const vitx_crossvit_config* cfg, vitx_crossvit_handle* out);
int32_t vitx_crossvit_destroy(vitx_crossvit_handle m);
int32_t vitx_crossvit_set_params(vitx_crossvit_handle m, const float* host_blob, int64_t n_elems);
int32_t vitx_crossvit_get_params(vitx_crossvit_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_crossvit_get_grads(vitx_crossvit_handle m, float* host_blob, int64_t n_elems);
/* device arenas (fp32, table order, every tensor 16-B aligned); call params_changed after writing the parameter arena */
int32_t vitx_crossvit_params_dev(vitx_crossvit_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_crossvit_grads_dev(vitx_crossvit_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_crossvit_params_changed(vitx_crossvit_handle m);
/* img [b, H, W, 3] NHWC, H and W <= image_size and divisible by both patch sizes; logits [b, num_classes] */
int32_t vitx_crossvit_forward(vitx_crossvit_handle m, const float* img_host, int32_t b, int32_t H, int32_t W, int32_t training, uint64_t seed,
                              float* logits_host);
int32_t vitx_crossvit_forward_dev(vitx_crossvit_handle m, const float* img_dev, int32_t b, int32_t H, int32_t W, int32_t training, uint64_t seed,
                                  float* logits_dev_or_null);
/* VJP of the last forward for d(logits): overwrites the gradient arena; optional d(img) */
int32_t vitx_crossvit_backward(vitx_crossvit_handle m, const float* dlogits_host, float* dimg_host_or_null);
int32_t vitx_crossvit_backward_dev(vitx_crossvit_handle m, const float* dlogits_dev, float* dimg_dev_or_null);
/* "sm_tokens" / "lg_tokens" [b, n, dim] (the multi-scale encoder's output), "sm_logits" / "lg_logits" [b, num_classes] */
int32_t vitx_crossvit_read(vitx_crossvit_handle m, const char* which, float* out_host, int64_t cap_elems, int64_t* n_elems);

/* ---- CCT (cct.py:307-345): convolutional tokenizer (Conv2D 'SAME' without bias, ReLU, MaxPool2D 'SAME', n_conv_layers times), optional
 * positional embedding, num_layers encoder blocks of the CCT form (one vitx_config.cct_block engine), LayerNorm, sequence pooling, fc.
 * A handle of its own; parameter order in DESIGN.md section 18.  Only the deterministic path (training falsy in the reference) exists. */
enum { VITX_CCT_POS_LEARNABLE = 0, VITX_CCT_POS_SINE = 1, VITX_CCT_POS_NONE = 2 };
typedef struct vitx_cct_config {
  int32_t img_height, img_width;   /* pair(img_size), cct.py:319 */
  int32_t n_input_channels, embedding_dim, n_conv_layers, kernel_size, stride, pooling_kernel_size, pooling_stride;
  int32_t num_layers, num_heads;
  int32_t dim_feedforward;         /* int(embedding_dim * mlp_ratio), cct.py:235 */
  int32_t num_classes;
  int32_t positional_embedding;    /* VITX_CCT_POS_*; SINE: a constant table built on the host, not a parameter */
  int32_t in_planes;               /* filters of every conv layer but the last; <= 0: 64 (cct.py:182) */
  float ln_eps;                    /* <= 0: Keras LayerNormalization default 1e-3 */
  int32_t compute;                 /* VITX_COMPUTE_*: the encoder blocks' mode; tokenizer, final norm, pooling and fc keep fp32 storage */
  int32_t max_batch;
  int32_t device_id;
  int32_t conv_chunk;              /* images per im2col + GEMM pass of the tokenizer; <= 0: sized from a fixed workspace budget */
  int32_t reserved[8];
} vitx_cct_config;
typedef struct vitx_cct* vitx_cct_handle;
/* host only, no GPU needed */
int32_t vitx_cct_param_table_size(const vitx_cct_config* cfg, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_cct_param_table_entry(const vitx_cct_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                   int64_t* offset_elems);
int32_t vitx_cct_sequence_length(const vitx_cct_config* cfg, int32_t* n_tokens);   /* the 'SAME' geometry rule, no tokenizer run */
int32_t vitx_cct_create(const vitx_cct_config* cfg, vitx_cct_handle* out);
int32_t vitx_cct_destroy(vitx_cct_handle m);
int32_t vitx_cct_set_params(vitx_cct_handle m, const float* host_blob, int64_t n_elems);
int32_t vitx_cct_get_params(vitx_cct_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_cct_get_grads(vitx_cct_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_cct_params_dev(vitx_cct_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_cct_grads_dev(vitx_cct_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_cct_params_changed(vitx_cct_handle m);
/* img [b, img_height, img_width, n_input_channels] NHWC; logits [b, num_classes] */
int32_t vitx_cct_forward(vitx_cct_handle m, const float* img_host, int32_t b, float* logits_host);
int32_t vitx_cct_forward_dev(vitx_cct_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null);
/* VJP of the last forward for d(logits): overwrites the gradient arena; d(img) only when asked for */
int32_t vitx_cct_backward(vitx_cct_handle m, const float* dlogits_host, float* dimg_host_or_null);
int32_t vitx_cct_backward_dev(vitx_cct_handle m, const float* dlogits_dev, float* dimg_dev_or_null);
/* per-kernel-class timing of the steps between the two calls, as vitx_profile_begin / _end: the blocks' classes plus the composite's own
 * (cct_im2col, cct_conv_gemm, cct_col2im, cct_relu_maxpool_fwd / _bwd, cct_seqpool_fwd / _bwd) */
int32_t vitx_cct_profile_begin(vitx_cct_handle m);
int32_t vitx_cct_profile_end(vitx_cct_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out);
/* "tokens" [b, n, dim] (the tokenizer's output), "encoded" [b, n, dim] (after the final norm), "pool_weights" [b, n], "pooled" [b, dim] */
int32_t vitx_cct_read(vitx_cct_handle m, const char* which, float* out_host, int64_t cap_elems, int64_t* n_elems);

/* ---- NesT (nest.py:150-216): patch embedding (Rearrange + 1x1 Conv2D = Dense, :178-181), then per hierarchy level the block partition
 * (:209) with the positional add (:140-142), block_repeats[i] transformer blocks on (b * blocks^2) sequences (one vitx_config.nest_block
 * engine per level), the inverse partition (:211) and, except at the last level, Aggregate (:111-123): Conv2D 3x3 'SAME' with bias, channel
 * LayerNorm, MaxPool2D 3/2 'SAME'; then LayerNorm, mean over the map, Dense (:196-200).  A handle of its own; parameter order in DESIGN.md
 * section 20.  Only the deterministic path (dropout 0) exists. */
typedef struct vitx_nest_config {
  int32_t image_size, patch_size, num_classes, dim, heads, num_hierarchies;   /* nest.py:151-157 */
  int32_t block_repeats[8];        /* cast_tuple(block_repeats, num_hierarchies), finest level first (nest.py:183); num_hierarchies <= 8 */
  int32_t mlp_mult;                /* nest.py:159 */
  float ln_eps;                    /* <= 0: nest.py:29's 1e-5 */
  int32_t compute;                 /* VITX_COMPUTE_*: the transformer blocks' mode; embedding, aggregation and head keep fp32 storage */
  int32_t max_batch;               /* images; level i's engine holds max_batch * 4^(H-1-i) sequences */
  int32_t device_id;
  int32_t conv_chunk;              /* images per im2col + GEMM pass of an aggregation; <= 0: sized from a fixed workspace budget */
  /* the plain small-head attention kernels (dim_head 16 / 32, <= 288 tokens).  0: where they measured faster than the materialised path at
   * the usage shape -- the BF16 mode (MFMA form); FP32_PARITY and BF16X3 (fp32 FMA form) keep the materialised path, which measured faster
   * there.  1: wherever they apply.  -1: nowhere. */
  int32_t small_attn;
  int32_t reserved[7];
} vitx_nest_config;
typedef struct vitx_nest* vitx_nest_handle;
/* host only, no GPU needed */
int32_t vitx_nest_param_table_size(const vitx_nest_config* cfg, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_nest_param_table_entry(const vitx_nest_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                    int64_t* offset_elems);
int32_t vitx_nest_create(const vitx_nest_config* cfg, vitx_nest_handle* out);
int32_t vitx_nest_destroy(vitx_nest_handle m);
int32_t vitx_nest_set_params(vitx_nest_handle m, const float* host_blob, int64_t n_elems);
int32_t vitx_nest_get_params(vitx_nest_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_nest_get_grads(vitx_nest_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_nest_params_dev(vitx_nest_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_nest_grads_dev(vitx_nest_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_nest_params_changed(vitx_nest_handle m);
/* img [b, image_size, image_size, 3] NHWC; logits [b, num_classes] */
int32_t vitx_nest_forward(vitx_nest_handle m, const float* img_host, int32_t b, float* logits_host);
int32_t vitx_nest_forward_dev(vitx_nest_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null);
/* VJP of the last forward for d(logits): overwrites the gradient arena; d(img) only when asked for */
int32_t vitx_nest_backward(vitx_nest_handle m, const float* dlogits_host, float* dimg_host_or_null);
int32_t vitx_nest_backward_dev(vitx_nest_handle m, const float* dlogits_dev, float* dimg_dev_or_null);
/* per-kernel-class timing of the steps between the two calls, as vitx_profile_begin / _end: every level's block classes (attn_small_fwd /
 * _bwd among them) plus the composite's own (nest_embed, nest_blocks, nest_im2col, nest_conv_gemm, nest_col2im, nest_maxpool_fwd / _bwd,
 * nest_head) */
int32_t vitx_nest_profile_begin(vitx_nest_handle m);
int32_t vitx_nest_profile_end(vitx_nest_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out);
/* "embedded" [b, f, f, dim]; "level.<i>" [b, f_i, f_i, d_i] (the level's output after un-blocking, before aggregation); "aggregated.<i>"
 * [b, f_{i+1}, f_{i+1}, d_{i+1}]; "pooled" [b, d_last] */
int32_t vitx_nest_read(vitx_nest_handle m, const char* which, float* out_host, int64_t cap_elems, int64_t* n_elems);

/* ---- TwinsSVT (twins_svt.py:215-268): four stages of PatchEmbedding ('b (h p1) (w p2) c -> b h w (c p1 p2)' + 1x1 Conv2D = Dense, :94-106),
 * Transformer(depth 1), PEG (x + depthwise Conv2D 'SAME' with bias, :108-115), Transformer(depth s_depth) (:252-259); then GlobalAvgPool2D
 * and Dense (:261-264).  A Transformer layer (:199-213) is local attention on local_patch_size windows (:117-156), MLP (:78-92), global
 * attention against a global_k-strided reduction of the map (:158-190), MLP, each x + f(LayerNorm_channel(x)) (:37-68); the last stage has
 * no local pair (has_local=False, :255,258).  Every attention has 8 heads of 64 (:118,159: TwinsSVT passes neither), every MLP mult 4.
 * The local pairs of a stage run on one vitx_config.nest_block engine over (b * windows) sequences, the global pairs on one
 * vitx_config.global_k engine over b sequences of the whole map.  A handle of its own; parameter order in DESIGN.md section 21.  Only the
 * deterministic path (dropout 0) exists. */
typedef struct vitx_twins_config {
  /* the map the handle is built for; both 0 is allowed for the host-only table calls (no parameter depends on the image size) */
  int32_t image_h, image_w;
  int32_t num_classes;              /* twins_svt.py:217 */
  int32_t emb_dim[4], patch_size[4], local_patch_size[4], global_k[4], depth[4];   /* s1..s4 (:218-237) */
  int32_t peg_kernel_size;          /* :238; odd */
  float ln_eps;                     /* <= 0: twins_svt.py:46's 1e-5 */
  int32_t compute;                  /* VITX_COMPUTE_*: the transformer blocks' mode; embeddings, PEG and head keep fp32 storage */
  int32_t max_batch;
  int32_t device_id;
  /* the few-key attention kernels of the global pairs (attn_fewkey.hip: bf16 mode, at most 64 keys; K and V staged once in LDS, no score tensor).
   * 0: where they measured faster than the materialised path at the usage shape -- on.  1: wherever they apply.  -1: nowhere. */
  int32_t fused_global_attn;
  int32_t reserved[7];
} vitx_twins_config;
typedef struct vitx_twins* vitx_twins_handle;
/* host only, no GPU needed */
int32_t vitx_twins_param_table_size(const vitx_twins_config* cfg, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_twins_param_table_entry(const vitx_twins_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                     int64_t* offset_elems);
int32_t vitx_twins_create(const vitx_twins_config* cfg, vitx_twins_handle* out);
int32_t vitx_twins_destroy(vitx_twins_handle m);
int32_t vitx_twins_set_params(vitx_twins_handle m, const float* host_blob, int64_t n_elems);
int32_t vitx_twins_get_params(vitx_twins_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_twins_get_grads(vitx_twins_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_twins_params_dev(vitx_twins_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_twins_grads_dev(vitx_twins_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_twins_params_changed(vitx_twins_handle m);
/* img [b, image_h, image_w, 3] NHWC; logits [b, num_classes] */
int32_t vitx_twins_forward(vitx_twins_handle m, const float* img_host, int32_t b, float* logits_host);
int32_t vitx_twins_forward_dev(vitx_twins_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null);
/* VJP of the last forward for d(logits): overwrites the gradient arena; d(img) only when asked for */
int32_t vitx_twins_backward(vitx_twins_handle m, const float* dlogits_host, float* dimg_host_or_null);
int32_t vitx_twins_backward_dev(vitx_twins_handle m, const float* dlogits_dev, float* dimg_dev_or_null);
/* per-kernel-class timing of the steps between the two calls, as vitx_profile_begin / _end: every engine's block classes plus the composite's
 * own (twins_embed, twins_windows, twins_peg_fwd / _bwd, twins_head) */
int32_t vitx_twins_profile_begin(vitx_twins_handle m);
int32_t vitx_twins_profile_end(vitx_twins_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out);
/* "embedded.<s>" (the stage's patch embedding), "pre_peg.<s>", "peg.<s>" (in front of / behind the PEG), "stage.<s>" (the stage's output), each
 * [b, H_s, W_s, emb_dim_s]; "pooled" [b, emb_dim_4] */
int32_t vitx_twins_read(vitx_twins_handle m, const char* which, float* out_host, int64_t cap_elems, int64_t* n_elems);

/* ---- CvT (cvt.py:149-202): three stages of Conv2D(emb_dim, emb_kernel, 'SAME', emb_stride) with bias (:187, im2col + GEMM), channel LayerNorm
 * (:30-43,188) and a Transformer (:129-147,189-191) of `depth` layers x + Attention(LayerNorm x), x + MLP(LayerNorm x); then GlobalAvgPool2D and
 * Dense (:195-198).  Attention (:94-127) projects q and kv through DepthWiseConv2d (:79-92) -- depthwise 'SAME' convolution of proj_kernel
 * (stride 1 for q, kv_proj_stride for kv), BatchNormalization (:85), pointwise Dense -- and attends heads of 64 (:130: CvT never passes
 * dim_head); to_out always projects (:106-109).  MLP (:63-77) is two 1x1 convolutions around the exact GELU (:23-28).  A stage's blocks run
 * on one vitx_config.conv_proj_kernel engine over b sequences of the whole map.  A handle of its own; parameter order in DESIGN.md section 22.
 * Only the deterministic path (dropout 0) exists.  BatchNormalization: a training forward normalises with the statistics of the call's whole
 * batch and has a VJP; an inference forward normalises with moving_mean / moving_variance of the table and has none (vitx_cvt_backward
 * returns VITX_ERR_UNSUPPORTED after it).  No forward updates the moving statistics; their gradients are zeros. */
typedef struct vitx_cvt_config {
  /* the image the handle is built for; both 0 is allowed for the host-only table calls (no parameter depends on the image size) */
  int32_t image_h, image_w;
  int32_t num_classes;              /* cvt.py:151 */
  /* s1..s3 (:152-175) */
  int32_t emb_dim[3], emb_kernel[3], emb_stride[3], proj_kernel[3], kv_proj_stride[3], heads[3], depth[3], mlp_mult[3];
  float ln_eps;                     /* <= 0: cvt.py:31's 1e-5 */
  float bn_eps;                     /* <= 0: cvt.py:85's 1e-5 */
  int32_t compute;                  /* VITX_COMPUTE_*: the transformer blocks' mode; embeddings and head keep fp32 storage */
  int32_t max_batch;
  int32_t device_id;
  /* the fused attention kernels of attn_fewkey.hip (bf16 mode, heads of 64; K and V of an (image, head) staged once in LDS, no score tensor): the
   * few-key ones for at most 64 keys and the many-key ones (key chunks of 64 with an online softmax; d(k) / d(v) per chunk and d(q) as two
   * launches) for 65 .. 320 keys.  0: per class, where they measured faster than the materialised path at the usage shape (DESIGN.md
   * section 22).  1: wherever they apply.  -1: nowhere.  More keys, and the fp32 / bf16x3 modes, take the materialised path. */
  int32_t fused_attn;
  int32_t reserved[8];
} vitx_cvt_config;
typedef struct vitx_cvt* vitx_cvt_handle;
/* host only, no GPU needed */
int32_t vitx_cvt_param_table_size(const vitx_cvt_config* cfg, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_cvt_param_table_entry(const vitx_cvt_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                   int64_t* offset_elems);
int32_t vitx_cvt_create(const vitx_cvt_config* cfg, vitx_cvt_handle* out);
int32_t vitx_cvt_destroy(vitx_cvt_handle m);
int32_t vitx_cvt_set_params(vitx_cvt_handle m, const float* host_blob, int64_t n_elems);
int32_t vitx_cvt_get_params(vitx_cvt_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_cvt_get_grads(vitx_cvt_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_cvt_params_dev(vitx_cvt_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_cvt_grads_dev(vitx_cvt_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_cvt_params_changed(vitx_cvt_handle m);
/* CvT.call(img, training) (cvt.py:200-202).  img [b, image_h, image_w, 3] NHWC; logits [b, num_classes]; training != 0: BatchNormalization on
 * the statistics of these b images (the reference's default), 0: on the moving statistics */
int32_t vitx_cvt_forward(vitx_cvt_handle m, const float* img_host, int32_t b, int32_t training, float* logits_host);
int32_t vitx_cvt_forward_dev(vitx_cvt_handle m, const float* img_dev, int32_t b, int32_t training, float* logits_dev_or_null);
/* VJP of the last training forward for d(logits): overwrites the gradient arena; d(img) only when asked for */
int32_t vitx_cvt_backward(vitx_cvt_handle m, const float* dlogits_host, float* dimg_host_or_null);
int32_t vitx_cvt_backward_dev(vitx_cvt_handle m, const float* dlogits_dev, float* dimg_dev_or_null);
/* per-kernel-class timing of the steps between the two calls, as vitx_profile_begin / _end: every engine's block classes (cvt_dwbn_fwd / _bwd
 * among them) plus the composite's own (cvt_im2col, cvt_conv_gemm, cvt_col2im, cvt_embed_norm, cvt_head) */
int32_t vitx_cvt_profile_begin(vitx_cvt_handle m);
int32_t vitx_cvt_profile_end(vitx_cvt_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out);
/* "embedded.<s>" (the stage's embedding behind its LayerNorm) and "stage.<s>" (its output), each [b, H_s, W_s, emb_dim_s]; "q_in.<s>.<l>"
 * [b, H_s, W_s, emb_dim_s] and "kv_in.<s>.<l>" [b, ceil(H_s / stride), ceil(W_s / stride), emb_dim_s] (the inputs of layer l's pointwise
 * projections, behind BatchNormalization, widened to fp32); "pooled" [b, emb_dim_3] */
int32_t vitx_cvt_read(vitx_cvt_handle m, const char* which, float* out_host, int64_t cap_elems, int64_t* n_elems);

/* ---- CrossFormer (crossformer.py:205-257): four stages of CrossEmbedLayer (:30-48: one Conv2D 'SAME' with bias per kernel size, kernel sizes
 * sorted, widths int(dim / 2^i) and the rest for the last, concatenated over channels; im2col + GEMM per scale) and a Transformer (:182-203) of
 * `depth` layers x + short_attn(x), x + MLP(x), x + long_attn(x), x + MLP(x); then the mean over the map and Dense (:245-248).  Attention
 * (:104-180) is a channel LayerNorm (eps 1e-5, :74-87), a window partition -- 'short': contiguous wsz x wsz windows (:144), 'long': the dilated
 * partition 'b (l1 h) (l2 w) d -> (b h w) l1 l2 d' (:146) --, heads of 32 (:105: CrossFormer never passes dim_head; heads = dim // 32),
 * softmax(scale q k^T + bias) v with the bias of the DynamicPositionBias network (:51-71) gathered through rel_pos_indices (:126-131,159-165),
 * and to_out.  The bias network receives no gradient in the reference (:163 leaves the tape through .numpy()): its gradients are zeros.
 * A stage's short pairs run on one vitx_config.nest_block engine over (b * windows) sequences of local^2 tokens, its long pairs on another over
 * sequences of global^2 tokens; the bias reaches the small-head attention kernels' BIAS form through the engines.  A handle of its own;
 * parameter order in DESIGN.md section 23.  Only the deterministic path (ff_dropout 0) exists; attn_dropout is unused by the reference. */
#define VITX_CF_MAX_SCALES 8
typedef struct vitx_crossformer_config {
  /* the image the handle is built for; both 0 is allowed for the host-only table calls (no parameter depends on the image size) */
  int32_t image_h, image_w;
  int32_t num_classes;              /* crossformer.py:213 */
  int32_t dim[4], depth[4], global_window_size[4], local_window_size[4];   /* :207-210 */
  int32_t n_kernels[4];             /* :211: kernel sizes per stage, 1 .. VITX_CF_MAX_SCALES (any order: the library sorts them as :34 does) */
  int32_t kernel_sizes[4][VITX_CF_MAX_SCALES];
  int32_t strides[4];               /* :212 */
  float ln_eps;                     /* <= 0: crossformer.py:75's 1e-5 */
  int32_t compute;                  /* VITX_COMPUTE_*: the transformer blocks' mode; embeddings, bias network and head keep fp32 */
  int32_t max_batch;
  int32_t device_id;
  /* the window attention kernels (attn_window.hip: bf16 mode, at most 64 tokens; one wave per (window, head), the bias staged in LDS, d(q, k, v)
   * written by the same wave).  0: where they measured faster than the BIAS form of the small-head kernels at the usage shape (DESIGN.md
   * section 23).  1: wherever they apply.  -1: nowhere.  More tokens, and the fp32 / bf16x3 modes, take the small-head kernels. */
  int32_t window_attn;
  int32_t reserved[7];
} vitx_crossformer_config;
typedef struct vitx_crossformer* vitx_crossformer_handle;
/* host only, no GPU needed */
int32_t vitx_crossformer_param_table_size(const vitx_crossformer_config* cfg, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_crossformer_param_table_entry(const vitx_crossformer_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4],
                                           int32_t* rank, int64_t* offset_elems);
int32_t vitx_crossformer_create(const vitx_crossformer_config* cfg, vitx_crossformer_handle* out);
int32_t vitx_crossformer_destroy(vitx_crossformer_handle m);
/* set_params / params_changed also evaluate every attention's bias network again (crossformer.py:159-163 does it per call; the bias is a
 * function of the parameters alone) */
int32_t vitx_crossformer_set_params(vitx_crossformer_handle m, const float* host_blob, int64_t n_elems);
int32_t vitx_crossformer_get_params(vitx_crossformer_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_crossformer_get_grads(vitx_crossformer_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_crossformer_params_dev(vitx_crossformer_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_crossformer_grads_dev(vitx_crossformer_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_crossformer_params_changed(vitx_crossformer_handle m);
/* CrossFormer.call (crossformer.py:250-257).  img [b, image_h, image_w, 3] NHWC; logits [b, num_classes] */
int32_t vitx_crossformer_forward(vitx_crossformer_handle m, const float* img_host, int32_t b, float* logits_host);
int32_t vitx_crossformer_forward_dev(vitx_crossformer_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null);
/* VJP of the last forward for d(logits): overwrites the gradient arena (the dpb.* entries with zeros, :163); d(img) only when asked for */
int32_t vitx_crossformer_backward(vitx_crossformer_handle m, const float* dlogits_host, float* dimg_host_or_null);
int32_t vitx_crossformer_backward_dev(vitx_crossformer_handle m, const float* dlogits_dev, float* dimg_dev_or_null);
/* per-kernel-class timing of the steps between the two calls, as vitx_profile_begin / _end: every engine's block classes (attn_small_fwd / _bwd
 * among them) plus the composite's own (cf_im2col, cf_conv_gemm, cf_col2im, cf_windows, cf_head) */
int32_t vitx_crossformer_profile_begin(vitx_crossformer_handle m);
int32_t vitx_crossformer_profile_end(vitx_crossformer_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out);
/* "embedded.<s>" (the stage's cross-scale embedding, :45-48) and "stage.<s>" (its output), each [b, H_s, W_s, dim_s]; "pooled" [b, dim_4];
 * "bias.<s>.<l>.short" / "bias.<s>.<l>.long": the [n, n] position bias of layer l's short / long attention (:163) */
int32_t vitx_crossformer_read(vitx_crossformer_handle m, const char* which, float* out_host, int64_t cap_elems, int64_t* n_elems);
/* The biased attention kernels alone, on host tensors, for tests and bisecting (crossformer.py:156-171 and its VJP on bf16 storage, heads of
 * 32): qkv [b, n, 3, h, 32], d_o [b, n, h * 32], bias [n, n]; window_kernel != 0: attn_window.hip (1 <= n <= 64), 0: the BIAS form of the
 * small-head kernels (n <= 288).  Every device activation buffer gets tail_rows extra rows behind its b * n live ones, filled with tail_value
 * (NaN allowed) before the run; o_host [(b * n + tail_rows), h * 32] and dqkv_host [(b * n + tail_rows), 3 * h * 32] return the whole buffers
 * (widened from bf16), so that a caller sees both that nothing past the live rows was read and that nothing past them was written;
 * lse_host [b, h, n]. */
int32_t vitx_crossformer_window_attn(vitx_crossformer_handle m, const float* qkv_host, const float* d_o_host, const float* bias_host, int32_t b, int32_t n,
                                     int32_t h, int32_t tail_rows, float tail_value, int32_t window_kernel, float* o_host, float* lse_host, float* dqkv_host);
/* the dilated partition kernel on a host tensor, for tests and bisecting: inverse == 0 is 'b (l1 h) (l2 w) c -> (b h w) (l1 l2) c' with
 * l1 = l2 = g (crossformer.py:146) of in [b, H, W, c]; inverse != 0 is the way back (:178) of in [(b h w), (l1 l2), c] */
int32_t vitx_crossformer_partition(vitx_crossformer_handle m, const float* in_host, float* out_host, int32_t b, int32_t H, int32_t W, int32_t g,
                                   int32_t c, int32_t inverse);

/* ---- RegionViT (regionvit.py:184-263): a local map (Conv2D 8x8 stride 4 'SAME', or three 3x3 convolutions with LayerNormalization and GELU
 * between them, :210-221) and a region map (the (c p1 p2) patches of local_patch_size * window_size pixels through a 1x1 convolution, :223-226);
 * per stage a Downsample (3x3 stride 2 'SAME', stages 2-4) applied to BOTH maps with the same kernel, an optional PEG on the local map, and an
 * R2LTransformer (:118-182): per layer the region tokens attend to each other, every window of the local map gets its region token prepended,
 * the windows run attention -- THE SAME Attention weights, plus the stage's learned relative position bias (an Embedding [(2 ws - 1)^2, 4],
 * shared by the stage's layers, zero for the region token) -- and the MLP, and the two are split again.  Attention is pre-norm with 4 heads of
 * 32 (:80).  Then mean over the region map, LayerNormalization, Dense (:243-247).  A stage drives two vitx_config.nest_block engines: one over
 * the (b * windows) sequences of 1 + window tokens with the per-head bias (small-head BIAS kernels or, bf16 with at most 64 tokens, the window
 * kernels), one over the b region sequences whose blocks stop behind the attention; both hold the layer's attention weights and the gradients
 * are summed.  The embedding's gradient is the sum over sequences and layers of dS, gathered back through the index.  A handle of its own;
 * parameter order in DESIGN.md section 26.  Only the deterministic path (ff_dropout 0) exists; attn_dropout is unused by the reference. */
typedef struct vitx_regionvit_config {
  /* the image the handle is built for; both 0 is allowed for the host-only table calls (no parameter depends on the image size) */
  int32_t image_h, image_w;
  int32_t num_classes;              /* regionvit.py:189 */
  int32_t dim[4], depth[4];         /* :186-187 */
  int32_t window_size;              /* :188 */
  int32_t local_patch_size;         /* :191 */
  int32_t tokenize_local_3_conv;    /* :190 */
  int32_t use_peg;                  /* :192 */
  float ln_eps;                     /* <= 0: Keras LayerNormalization's 1e-3 */
  int32_t compute;                  /* VITX_COMPUTE_*: the transformer blocks' mode; encoders, Downsample, PEG and head keep fp32 */
  int32_t max_batch;
  int32_t device_id;
  /* the window attention kernels (attn_window.hip) for the window sequences of at most 64 tokens in the bf16 mode.  0: the measured default
   * (DESIGN.md section 26).  1: wherever they apply.  -1: nowhere.  More tokens, and the fp32 / bf16x3 modes, take the small-head kernels. */
  int32_t window_attn;
  int32_t reserved[7];
} vitx_regionvit_config;
typedef struct vitx_regionvit* vitx_regionvit_handle;
/* host only, no GPU needed */
int32_t vitx_regionvit_param_table_size(const vitx_regionvit_config* cfg, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_regionvit_param_table_entry(const vitx_regionvit_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4],
                                         int32_t* rank, int64_t* offset_elems);
int32_t vitx_regionvit_create(const vitx_regionvit_config* cfg, vitx_regionvit_handle* out);
int32_t vitx_regionvit_destroy(vitx_regionvit_handle m);
/* set_params / params_changed also gather every stage's position bias from its embedding table again */
int32_t vitx_regionvit_set_params(vitx_regionvit_handle m, const float* host_blob, int64_t n_elems);
int32_t vitx_regionvit_get_params(vitx_regionvit_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_regionvit_get_grads(vitx_regionvit_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_regionvit_params_dev(vitx_regionvit_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_regionvit_grads_dev(vitx_regionvit_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_regionvit_params_changed(vitx_regionvit_handle m);
/* RegionViT.call (regionvit.py:249-263).  img [b, image_h, image_w, 3] NHWC; logits [b, num_classes] */
int32_t vitx_regionvit_forward(vitx_regionvit_handle m, const float* img_host, int32_t b, float* logits_host);
int32_t vitx_regionvit_forward_dev(vitx_regionvit_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null);
/* VJP of the last forward for d(logits): overwrites the gradient arena; d(img) only when asked for */
int32_t vitx_regionvit_backward(vitx_regionvit_handle m, const float* dlogits_host, float* dimg_host_or_null);
int32_t vitx_regionvit_backward_dev(vitx_regionvit_handle m, const float* dlogits_dev, float* dimg_dev_or_null);
/* per-kernel-class timing as vitx_profile_begin / _end: every engine's block classes (attn_window_* / attn_small_*, attn_dbias among them) plus
 * the composite's own (rv_im2col, rv_conv_gemm, rv_col2im, rv_windows, rv_peg, rv_encoder, rv_bias, rv_head) */
int32_t vitx_regionvit_profile_begin(vitx_regionvit_handle m);
int32_t vitx_regionvit_profile_end(vitx_regionvit_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out);
/* "local.<s>" [b, lh_s, lw_s, dim_s] and "region.<s>" [b, rh_s, rw_s, dim_s]: the maps behind stage s; "bias.<s>" [4, n, n]: the stage's
 * position bias as the attention adds it (n = 1 + window tokens; a stage without layers has none); "pooled" [b, dim_4] */
int32_t vitx_regionvit_read(vitx_regionvit_handle m, const char* which, float* out_host, int64_t cap_elems, int64_t* n_elems);
/* One biased attention alone with a per-head bias, on host tensors, for tests and bisecting (bf16 storage, heads of 32): qkv [b, n, 3, h, 32],
 * d_o [b, n, h * 32], bias [h, n, n]; window_kernel != 0: attn_window.hip (1 <= n <= 64), 0: the BIAS form of the small-head kernels
 * (n <= 288).  Tail rows as vitx_crossformer_window_attn.  dbias_host [h, n, n]: the sum over the b sequences of dS. */
int32_t vitx_regionvit_attn(vitx_regionvit_handle m, const float* qkv_host, const float* d_o_host, const float* bias_host, int32_t b, int32_t n, int32_t h,
                            int32_t tail_rows, float tail_value, int32_t window_kernel, float* o_host, float* lse_host, float* dqkv_host,
                            float* dbias_host);
/* the window partition kernels on host tensors: inverse == 0 joins region [b, rh, rw, c] and local [b, rh * wh, rw * ww, c] into
 * tokens [(b rh rw), 1 + wh * ww, c]; inverse != 0 splits tokens back into the two */
int32_t vitx_regionvit_partition(vitx_regionvit_handle m, float* region_host, float* local_host, float* tokens_host, int32_t b, int32_t rh, int32_t rw,
                                 int32_t wh, int32_t ww, int32_t c, int32_t inverse);

/* ---- PiT (pit.py:158-219): Unfold(patch_size, stride patch_size // 2) + Dense (:110-122,179-182: overlapping 'VALID' patches in (kh, kw, c)
 * order), the class token and the position rows (:211-213), one Transformer (:91-108) per entry of zip(depth, heads) -- pre-norm Attention
 * (heads of dim_head, to_out absent when heads == 1 and dim_head == dim, :59) and MLP -- and LayerNormalization + Dense on row 0
 * (:202-205,217).  Each stage with layers runs on one ordinary vitx_config engine (VITX_VARIANT_VIT), so vitx_pit_set_long_attn applies.
 * pit.py:194 `not_last = ind < (len(depth) < 1)` is never true: the reference never inserts its Pool (:140-156) and never doubles dim.
 * pool_stages == 0 reproduces that.  pool_stages != 0 runs the loop body of :196-200 with not_last true: behind every stage but the last a
 * Pool(dim) -- Dense dim -> 2 dim on the class row (:148), Conv2D(2 dim, 3, strides 2, 'SAME', groups = dim) with bias and a 1x1 Conv2D with
 * bias (:130-131) on the other rows as a square map -- and dim doubled; mlp_dim and dim_head stay.  A handle of its own; parameter order in
 * DESIGN.md section 27.  Only the deterministic path (dropout 0) exists. */
#define VITX_PIT_MAX_STAGES 8
typedef struct vitx_pit_config {
  /* the image the handle is built for; both 0 is allowed for the host-only table calls */
  int32_t image_h, image_w;
  int32_t image_size;               /* pit.py:160: sizes pos_embedding [1, conv_output_size(image_size, patch_size, patch_size // 2)^2 + 1, dim] (:184-187) */
  int32_t patch_size;               /* :161 */
  int32_t num_classes;              /* :162 */
  int32_t dim;                      /* :163 */
  int32_t n_stages;                 /* the length of zip(depth, cast_tuple(heads, len(depth))) (:177,193) */
  int32_t depth[VITX_PIT_MAX_STAGES], heads[VITX_PIT_MAX_STAGES];   /* :164-165; a depth of 0 is a stage without layers */
  int32_t mlp_dim, dim_head;        /* :166-167 */
  int32_t pool_stages;              /* 0: the reference (no Pool); != 0: Pool(dim) behind every stage but the last */
  float ln_eps;                     /* <= 0: Keras LayerNormalization's 1e-3 */
  int32_t compute;                  /* VITX_COMPUTE_*: the transformer blocks' mode; tokenizer, Pool and head keep fp32 storage */
  int32_t max_batch;
  int32_t device_id;
  int32_t long_attn;                /* != 0: vitx_pit_set_long_attn(handle, 1) at creation */
  int32_t reserved[8];
} vitx_pit_config;
typedef struct vitx_pit* vitx_pit_handle;
/* host only, no GPU needed */
int32_t vitx_pit_param_table_size(const vitx_pit_config* cfg, int64_t* n_tensors, int64_t* n_elems);
int32_t vitx_pit_param_table_entry(const vitx_pit_config* cfg, int64_t index, char* name, int32_t name_cap, int64_t shape[4], int32_t* rank,
                                   int64_t* offset_elems);
int32_t vitx_pit_create(const vitx_pit_config* cfg, vitx_pit_handle* out);
int32_t vitx_pit_destroy(vitx_pit_handle m);
int32_t vitx_pit_set_params(vitx_pit_handle m, const float* host_blob, int64_t n_elems);
int32_t vitx_pit_get_params(vitx_pit_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_pit_get_grads(vitx_pit_handle m, float* host_blob, int64_t n_elems);
int32_t vitx_pit_params_dev(vitx_pit_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_pit_grads_dev(vitx_pit_handle m, float** dev_ptr, int64_t* n_elems);
int32_t vitx_pit_params_changed(vitx_pit_handle m);
/* vitx_set_long_attn on every stage's engine (the streamed-key attention past 288 tokens; bf16, dim_head 64); the first refusal is returned */
int32_t vitx_pit_set_long_attn(vitx_pit_handle m, int32_t on);
/* PiT.call (pit.py:207-219).  img [b, image_h, image_w, 3] NHWC; logits [b, num_classes] */
int32_t vitx_pit_forward(vitx_pit_handle m, const float* img_host, int32_t b, float* logits_host);
int32_t vitx_pit_forward_dev(vitx_pit_handle m, const float* img_dev, int32_t b, float* logits_dev_or_null);
/* VJP of the last forward for d(logits): overwrites the gradient arena (pos_embedding rows the image does not use: zeros); d(img) only when
 * asked for */
int32_t vitx_pit_backward(vitx_pit_handle m, const float* dlogits_host, float* dimg_host_or_null);
int32_t vitx_pit_backward_dev(vitx_pit_handle m, const float* dlogits_dev, float* dimg_dev_or_null);
/* Pool.call (pit.py:146-156) of the Pool behind `stage` alone, on host tokens [b, n, dim_stage] with n = 1 + h * h at most the stage's own token
 * count: out [b, 1 + ceil(h / 2)^2, 2 dim_stage].  A handle whose stages all have depth 0 is one of pools alone.  pool_backward is the VJP of
 * the last pool_forward: dout as out; it writes that Pool's six entries of the gradient arena (vitx_pit_get_grads) and, when asked for,
 * d(tokens).  Both invalidate the state of a model forward. */
int32_t vitx_pit_pool_forward(vitx_pit_handle m, int32_t stage, const float* tokens_host, int32_t b, int32_t n, float* out_host);
int32_t vitx_pit_pool_backward(vitx_pit_handle m, int32_t stage, const float* dout_host, float* dtokens_host_or_null);
/* per-kernel-class timing as vitx_profile_begin / _end: every engine's block classes plus the composite's own (pit_unfold, pit_embed,
 * pit_pool_fwd, pit_pool_bwd, pit_head).  A handle without an engine profiles nothing. */
int32_t vitx_pit_profile_begin(vitx_pit_handle m);
int32_t vitx_pit_profile_end(vitx_pit_handle m, vitx_kernel_stat* out, int32_t cap, int32_t* n_out);
/* "tokens" [b, n_0, dim] (behind the position rows), "stage.<s>" [b, n_s, dim_s] (the stage's output), "pooled.<s>" [b, n_{s+1}, 2 dim_s] (the
 * Pool behind stage s) */
int32_t vitx_pit_read(vitx_pit_handle m, const char* which, float* out_host, int64_t cap_elems, int64_t* n_elems);

#ifdef __cplusplus
}
#endif
#endif /* VITX_H_ */
