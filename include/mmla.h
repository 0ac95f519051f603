/*
 * mmla.h -- C ABI of the MI355X-native mmla-audio hot path (libmmla.so).
 *
 * The reference (lizaibeim/mmla-audio) has no FFI of its own: its per-clip path is a set of plain
 * Python functions over librosa / python_speech_features / TensorFlow.  Each entry
 * point below replaces one of those call sites; the Python drop-in shim (mmla_audio_amd/) binds them
 * with ctypes under the reference's own names (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - Every function returns MMLA_OK (0) or a negative MMLA_E_* code; the message is in
 *     mmla_last_error(ctx).  Nothing throws across the ABI.
 *   - Buffers are caller-owned.  By default they are HOST pointers (the call copies in and out and
 *     is synchronous).  With MMLA_DEVICE_PTR they are device pointers on the context's GPU and the
 *     call only enqueues work on the context stream (mmla_set_stream), returning immediately.
 *   - A context is not thread-safe: use one per thread / per GPU.  The multi-GPU driver (one process
 *     per GPU, RCCL all-gather of logits) lives above this ABI.
 *   - PCM is 16 kHz mono int16; clip c starts at pcm + c * clip_stride (in samples) and has
 *     lens[c] valid samples (lens == NULL: every clip has clip_len samples).  Without lens the
 *     stride may be smaller than clip_len: overlapping windows of one signal (the offline
 *     segmentation of overlap_detection_post_processing.py:23-85 with step < window).  Only the
 *     mmla_capture_* and mmla_*_pipeline_capture calls take another rate or interleaved channels.
 */
#ifndef MMLA_H_
#define MMLA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMLA_ABI_VERSION 2

enum mmla_status {
  MMLA_OK = 0,
  MMLA_E_INVALID = -1,   /* bad argument (null pointer, negative size, unknown model kind) */
  MMLA_E_HIP = -2,       /* HIP runtime error */
  MMLA_E_NOWEIGHTS = -3, /* forward called before mmla_load_weights for that model */
  MMLA_E_OOM = -4,       /* device allocation failed */
  MMLA_E_SHAPE = -5,     /* packed weight blob has the wrong number of floats */
  MMLA_E_RANGE = -6      /* 3xFP16: an operand left the fp16 range in a device-pointer call */
};

enum mmla_model { MMLA_MODEL_OD = 0, MMLA_MODEL_SI = 1 };
enum mmla_head { MMLA_HEAD_SOFTMAX = 0, MMLA_HEAD_SIGMOID = 1 };

#define MMLA_DEVICE_PTR 0x1u /* data pointers are device pointers; call is asynchronous */
/* the calls that take nr_passes (mmla_condition, mmla_{od,si,room}_pipeline_conditioned,
 * mmla_od_pipeline_gated): the passes run the non-stationary gate of mmla_nr_reduce_ns */
#define MMLA_NR_NONSTATIONARY 0x2u
/*
 * The feature images of the OD detector (overlap_features_generator.py:119-177), all [128,151,3] u8 of the
 * same normalised log-mel, rows flipped (origin="lower"):
 *   MMLA_OD_IMG_ZCR     generate_zcr_image: R = trunc(255 zcr), G = B = trunc(255 (1 - norm))
 *   MMLA_OD_IMG_GRAY    generate_gary_image(cmap="gray"): plt.imsave's pixel LUT_gray[min(trunc(256 norm), 255)],
 *                       written R = G = B as decode_png(png, 3) reads it (decode_png(png, 1) gives that byte)
 *   MMLA_OD_IMG_VIRIDIS generate_viridis_image: LUT_viridis[min(trunc(256 norm), 255)]
 * LUT = matplotlib.colormaps[name](np.arange(256), bytes=True)[:, :3] (matplotlib 3.10.8; the gray table is
 * not the identity).  No autoscale: the clip's normalised minimum and maximum are 0 and 1.  A NaN pixel
 * (digital silence) is (0, 0, 0): imsave's RGBA (0, 0, 0, 0).
 * mmla_od_features, mmla_od_features_f32 (strided and device-pointer calls alike) take the type in two flag
 * bits, MMLA_OD_IMG_FLAGS(type): none set = ZCR, both set = MMLA_E_INVALID.  The pipelines make the
 * loaded model's type (mmla_od_set_image_type).
 */
#define MMLA_OD_IMG_ZCR 0
#define MMLA_OD_IMG_GRAY 1
#define MMLA_OD_IMG_VIRIDIS 2
#define MMLA_OD_IMG_SHIFT 4
#define MMLA_OD_IMG_MASK (0x3u << MMLA_OD_IMG_SHIFT)
#define MMLA_OD_IMG_FLAGS(type) ((uint32_t)(type) << MMLA_OD_IMG_SHIFT)

/* OD front-end geometry (overlap_features_generator.py:39-42,73-81) */
#define MMLA_OD_MELS 128
#define MMLA_OD_FRAMES 151
#define MMLA_OD_CLIP 24000
/* SI front-end geometry (speaker_identification.py:386-395) */
#define MMLA_SI_FRAMES 256
#define MMLA_SI_DIMS 39
#define MMLA_SI_SILENT_LEN 4000
/* speaker registration (speaker_identification.py:401-432): width of the embedding the sigmoid head is
 * trained on, and the largest head mmla_si_head_fit trains */
#define MMLA_SI_EMBED 512
#define MMLA_SI_TRAIN_MAX_CLASSES 32

typedef struct mmla_ctx mmla_ctx;

int mmla_abi_version(void);

/* CRC-32C (Castagnoli) of n bytes -> *crc (host only, no context or device): the checksum TF's
 * tensor bundle stores per tensor (BundleEntryProto.crc32c, masked as LevelDB does; tfbundle.py
 * verifies every tensor it loads from variables.data-*, replacing the check of
 * tf.keras.models.load_model at record_on_pc.py:88 / SI record_on_pc.py:77). */
int mmla_crc32c(const void* data, int64_t n, uint32_t* crc);

/* PNG scanline reconstruction (host only, no context or device): `raw` is the inflated IDAT stream
 * of a non-interlaced image, h rows of 1 filter-type byte + row_bytes bytes; `bpp` = bytes per
 * complete pixel (>= 1; 1 for sub-byte depths).  Undoes filters 0-4 (None, Sub, Up, Average, Paeth;
 * PNG spec section 9) into out[h * row_bytes].  MMLA_E_INVALID on an unknown filter type.  Replaces
 * libpng's row reconstruction inside tf.image.decode_png (record_on_pc.py:157,
 * overlap_detection_post_processing.py:205; mmla_audio_amd/tf_compat/image.py). */
int mmla_png_unfilter(const uint8_t* raw, int64_t h, int64_t row_bytes, int32_t bpp, uint8_t* out);

/* Test hook: the colour map compiled into the front-end for image type MMLA_OD_IMG_GRAY (1) or MMLA_OD_IMG_VIRIDIS (2) (host
 * only, no context or device): rgb [256][3] u8 = matplotlib.colormaps[name](np.arange(256), bytes=True)[:, :3].
 * MMLA_E_INVALID for any other type. */
int mmla_debug_od_image_lut(int32_t type, uint8_t* rgb);

/* Create a context on HIP device `device` (owns a stream, device workspaces and loaded weights). */
int mmla_create(int device, mmla_ctx** out);
int mmla_destroy(mmla_ctx* ctx);
const char* mmla_last_error(const mmla_ctx* ctx);
/* Use an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the context's
 * own stream, a blocking stream (it orders with the legacy NULL stream, i.e. with PyTorch's default
 * stream; work on any other stream that produces a call's device inputs must be ordered by the
 * caller, e.g. by passing that stream here).  The new stream first waits (hipStreamWaitEvent) for
 * the work already enqueued on the old one, which still uses this context's workspaces. */
int mmla_set_stream(mmla_ctx* ctx, void* hip_stream);
/* Wait for the context stream; returns MMLA_E_RANGE (see mmla_range_check) if a device-pointer call
 * since the last check overflowed the fp16 range, MMLA_E_HIP if one ran the split BiLSTM (batches of
 * <= 128 clips) and a workgroup of it timed out (NaN probabilities; host-pointer calls re-run such a
 * micro-batch on the unsplit kernel instead, bit-identical). */
int mmla_synchronize(mmla_ctx* ctx);
/*
 * Arithmetic of the spatial convolutions (98 % of OD-NET FLOPs) and the BiLSTM:
 *   MMLA_PREC_F16X3 (default) error-compensated 3xFP16 on f16 MFMA: operands split hi + 2^-11 lo,
 *                   hi*hi + hi*lo + lo*hi accumulated in f32 (~22-bit products, f32 accumulation);
 *                   needs |activation| < 4094 (65504 / 2^4) at every conv operand -- the fused
 *                   res_blocks and the halo-tiled convs alike split x 2^4 and compare the scaled
 *                   value with 65504 -- and < 1023.5 at the LSTM input (x 2^6).  Each weight tensor is split
 *                   at its own power-of-two scale (2^8 for max |w| in [1/16, 255.9), else the one
 *                   putting max |w| in [2^13, 2^14)), so any finite checkpoint stays on this path;
 *                   a tensor holding inf / NaN makes that model run exact f32 (decided at
 *                   mmla_load_weights).  Range guard: every kernel that splits an activation flags
 *                   a value outside its range.  Host-pointer calls then re-run the micro-batch in exact f32
 *                   (counted by mmla_range_check); device-pointer calls report MMLA_E_RANGE from
 *                   the next mmla_range_check / mmla_synchronize.
 *                   A NaN or an inf in a caller's float input (an image of mmla_od_forward, the
 *                   features of mmla_si_forward / mmla_si_embed) is out of range like any other
 *                   value: the kernel that reads the input flags it.  A host-pointer call then
 *                   returns what exact f32 gives -- NaN for that clip, as the float64 reference
 *                   network does, and the other clips' exact-f32 results --; a device-pointer call
 *                   reports MMLA_E_RANGE.  MMLA_PREC_F32 returns NaN for such a clip as well: its
 *                   ReLU and max-pools keep NaN.
 *   MMLA_PREC_F32   exact f32 MFMA (v_mfma_f32_32x32x2_f32), 1/5.3 of the throughput.
 * The front-ends (OD f32, SI f64), the OD stem Conv2D(1x1), the OD Dense(K) head and the softmax /
 * sigmoid are the same in both modes; under MMLA_PREC_F16X3 the strided 1x1 shortcuts (OD blocks 1,
 * 4, 7; SI pool units) and the SI Dense(K) run 3xFP16 with the convolutions they are fused into.
 */
enum mmla_precision { MMLA_PREC_F32 = 0, MMLA_PREC_F16X3 = 1 };
int mmla_set_precision(mmla_ctx* ctx, int mode);
/* Waits for the context stream.  *f32_reruns (nullable) = host-pointer micro-batches re-run in
 * exact f32 so far; returns MMLA_E_RANGE (and clears the flag) if a device-pointer call since the
 * last check split an out-of-range operand -- its results are invalid. */
int mmla_range_check(mmla_ctx* ctx, int64_t* f32_reruns);
/*
 * Clips per internal micro-batch (activation memory).  0 = sized at each call from the device's
 * free memory, capped at 16384 (OD) / 65536 (SI) clips; an allocation failure halves it and
 * retries.  Per-clip device footprint of a micro-batch: OD ~7.6 MB (three n*128*151*32 f32
 * activation buffers + image + front-end scratch), so the 16384-clip default holds ~124 GB;
 * SI ~0.14 MB (65536 clips ~9 GB).  Weights: OD ~12 MB, SI ~10 MB.  Workspaces are kept for
 * reuse until mmla_release_workspace or mmla_destroy.  mmla_od_pipeline_gated with nr_passes > 0 adds
 * per clip the second image (58 KB) and two float clip buffers (2 x 4 x min(clip_len, 24000) bytes,
 * 192 KB; the output slots hold 4 K + 5 bytes per clip for the K classes of the loaded OD model), and per
 * launch of the noise gate (at most 512 clips) ~6.9 MB of gate scratch per clip.
 * mmla_condition and the conditioned pipelines add per clip two float buffers and one int16 buffer of
 * clip_len samples (10 x clip_len bytes: 0.41 MB at 40960), a byte per 30 ms frame, and the gate's
 * scratch (~8.3 MB per clip at 40960 samples, at most 512 clips at a time); their micro-batches are
 * multiples of items_per_stream (at least one stream, even where a smaller size was set here).
 * mmla_od_pipeline_mixed adds per clip the mixed-clip buffer (24000 int16: 48 KB) and 4 bytes of length,
 * and per host-pointer call the pool and the plan (160 bytes per clip), which stay until
 * mmla_release_workspace; a host-pointer mmla_od_mix holds the same (2 x clip_len bytes per clip).
 * mmla_od_forward / _u8 with a one-channel model (mmla_od_image) widen the caller's [.,1] images into the
 * three-channel image buffer above; a host-pointer call adds the staged one-channel images per clip (19 KB
 * u8, 77 KB float).
 */
int mmla_set_microbatch(mmla_ctx* ctx, int64_t od_clips, int64_t si_clips);
/* The micro-batch sizes the next call would use. */
int mmla_get_microbatch(mmla_ctx* ctx, int64_t* od_clips, int64_t* si_clips);
/* Free every device workspace of the context (after its stream drains). */
int mmla_release_workspace(mmla_ctx* ctx);

/*
 * Load network weights from the packed float32 blob (host memory) in the canonical order of
 * mmla_audio_amd/weights.py spec(): ascending Keras `layer_with_weights-k`; conv/dense = kernel,
 * bias; BatchNorm = gamma, beta, moving_mean, moving_variance; Bidirectional LSTM = forward
 * kernel, recurrent_kernel, bias, backward kernel, recurrent_kernel, bias.  Keras layouts.
 * Replaces tf.keras.models.load_model(...) (record_on_pc.py:88; SI record_on_pc.py:77).
 * n_classes: OD = the K of the Dense(K) softmax head, 2 (the deployed timit2.0 model) .. MMLA_OD_MAX_CLASSES
 *            (the reference's research models have 3: overlap_detector.py:394, tfl_convert.py:13-34); SI =
 *            630 (base model) or N speakers (deployed head).
 * OD: n_floats must be that K's blob, weights.od_spec(K): the two-class blob with the last two tensors
 * [512, K] and [K].  K outside the range, or for K > 2 another n_floats, is MMLA_E_INVALID and the loaded
 * model stays (a two-class blob of another size: MMLA_E_SHAPE, as before).  Loading a model with another K
 * replaces the head: every OD inference entry -- mmla_od_forward, _u8, mmla_od_pipeline, _gated,
 * _conditioned, _mixed, _capture, mmla_room_pipeline_conditioned, _capture -- writes probs [n, K] with the
 * loaded K (mmla_od_classes), and argmax is the first index whose probability is above every earlier one.
 * head: MMLA_HEAD_SOFTMAX (base Dense(630, softmax), speaker_identification.py:215) or
 *       MMLA_HEAD_SIGMOID (deployed customized_dense, speaker_identification.py:409).
 */
#define MMLA_OD_MAX_CLASSES 8
int mmla_load_weights(mmla_ctx* ctx, int model_kind, const float* packed, int64_t n_floats,
                      int32_t n_classes, int32_t head);
/* *k = the classes of the loaded OD model.  MMLA_E_NOWEIGHTS before an OD model is loaded. */
int mmla_od_classes(mmla_ctx* ctx, int32_t* k);
/*
 * The image type of the loaded OD model (MMLA_OD_IMG_*): what every pipeline entry that runs the front-end
 * in front of OD-NET produces -- mmla_od_pipeline, _conditioned, _mixed, _capture,
 * mmla_room_pipeline_conditioned, _capture.  It is a property of the loaded model: mmla_load_weights
 * resets it to ZCR for a three-channel model (stem [1,1,3,16]) and to GRAY for a one-channel model (stem
 * [1,1,1,16], OverlapDetector(imagetype='gray'), overlap_detector.py:84-90).  A three-channel model takes
 * all three types (a gray PNG read with three channels is a legitimate input); a one-channel model only
 * GRAY, anything else is MMLA_E_INVALID.  MMLA_E_NOWEIGHTS before an OD model is loaded.
 * mmla_od_image: *type and *channels (both nullable) of the loaded model.
 * One-channel models: a blob whose stem kernel is [1,1,1,16] is 32 floats shorter than
 * weights.od_spec(K); 513 K - 32 is no multiple of 513, so mmla_load_weights tells (K, channels) from
 * n_floats.  mmla_od_forward / _u8 then take [n,128,151,1] (float / u8).  The device keeps 3 bytes per
 * pixel: the stem is stored with two zero rows and a caller's image is widened to (g, g, g) as it
 * enters; the fused pipelines need no widening, the front-end writes R = G = B.
 */
int mmla_od_set_image_type(mmla_ctx* ctx, int32_t type);
int mmla_od_image(mmla_ctx* ctx, int32_t* type, int32_t* channels);

/*
 * OverlapDetection front-end, replaces OverlapFeaturesGenerator.generate_mels / generate_zcr /
 * generate_zcr_image + the PNG round trip (overlap_features_generator.py:65-151;
 * record_on_pc.py:156-158).  Per clip (first 24000 samples, zero-padded if shorter):
 *   db      [n,128,151] f32  power_to_db(melspectrogram, ref=max, top_db=80)   (nullable)
 *   norm_db [n,128,151] f32  normalize_matrix(db) in [0,1] (NaN for digital silence) (nullable)
 *   zcr     [n,151]     f32  zero_crossing_rate(frame 400, hop 160)                 (nullable)
 *   img     [n,128,151,3] u8 the decoded PNG the model reads: rows flipped
 *                            (origin="lower"), R = trunc(255*zcr), G = B = trunc(255*(1-norm));
 *                            with MMLA_OD_IMG_FLAGS(type) in flags the gray or viridis image instead
 *                            (MMLA_OD_IMG_* above)                                  (nullable)
 */
int mmla_od_features(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                     const int32_t* lens, int32_t clip_len, float* db, float* norm_db, float* zcr,
                     uint8_t* img, uint32_t flags);
/* Same on float PCM in librosa.load's scale (y = x / 32768 for 16-bit files; |y| < 8188, since y 2^3 is
 * split into fp16 hi + lo -- a host call with a larger or non-finite sample in the read window returns
 * MMLA_E_RANGE, a device-pointer call reports it from the next mmla_range_check / mmla_synchronize): the
 * drop-in's path for what librosa.load(path, sr=None, mono=True) returns from a WAV that is not
 * 16-bit mono (stereo downmixed by the channel mean, 8/24/32-bit and float files) --
 * overlap_features_generator.py:72,93.  Zero crossings treat |y| <= 1e-10 as 0, as librosa. */
int mmla_od_features_f32(mmla_ctx* ctx, const float* y, int64_t n_clips, int64_t clip_stride,
                         const int32_t* lens, int32_t clip_len, float* db, float* norm_db,
                         float* zcr, uint8_t* img, uint32_t flags);

/*
 * SpeakerIdentification front-end, replaces input_feature_gen (speaker_identification.py:372-398):
 * psf.mfcc(winlen .025, winstep .01, nfft 512) -> delta(.,2) -> delta(delta,2) -> [T,39] ->
 * zero-pad / truncate to 256 frames.  Clips with lens < 4000 are 'silent': silent[c] = 1 and
 * feat[c] is all zeros.  feat [n,256,39] f32 (float64 arithmetic inside); silent [n] u8 (nullable).
 */
int mmla_si_features(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                     const int32_t* lens, int32_t clip_len, float* feat, uint8_t* silent,
                     uint32_t flags);

/*
 * Whole-signal SI features cut into 256-frame windows, replaces the conversation-level MFCC +
 * deltas + chunking of speaker_identification_post_processing.py:255-269 and
 * make_feature_experiment (speaker_identification.py:340-353).  pcm [n_samples] int16; window s
 * holds global frames [256 s, 256 s + 256) (deltas edge-padded at the true sequence ends, zero
 * rows past the last frame).  n_windows must be ceil(T / 256), T = psf frame count of n_samples.
 * feat [n_windows, 256, 39] f32.
 */
int mmla_si_features_seq(mmla_ctx* ctx, const int16_t* pcm, int64_t n_samples, int64_t n_windows,
                         float* feat, uint32_t flags);

/*
 * mmla_si_features_seq on a ragged batch of signals in one launch: the front-end of registration, where
 * every speaker's recording is cut into 256-frame windows (make_feature_experiment,
 * speaker_identification.py:317-369).  Signal i = pcm + i * stride has lens[i] samples (nullable:
 * clip_len; stride >= clip_len for more than one signal).  With T(n) = 1 for 1 <= n <= 400, else
 * 1 + ceil((n - 400) / 160), w_max = ceil(T(clip_len) / 256):
 *   feat [n_signals, w_max, 256, 39] f32: window w < n_windows[i] = ceil(T(lens[i]) / 256) holds exactly
 *     what mmla_si_features_seq gives for that signal alone (global frames [256 w, 256 w + 256), deltas
 *     edge-padded at the signal's own ends, zero rows past its last frame); every other window, and
 *     every window of a signal with lens[i] == 0, is all zeros;
 *   n_windows [n_signals] i32 (nullable), 0 for an empty signal.
 * Host or device pointers (MMLA_DEVICE_PTR).  MMLA_E_INVALID: clip_len < 1, a host lens[i] outside
 * [0, clip_len] or above the stride (device pointers: clamped into [0, clip_len] by the kernel, the
 * convention of the VAD's lens).
 */
int mmla_si_features_seq_batch(mmla_ctx* ctx, const int16_t* pcm, int64_t n_signals, int64_t stride,
                               const int32_t* lens, int32_t clip_len, float* feat, int32_t* n_windows,
                               uint32_t flags);

/* OD-NET predict on float NHWC [n,128,151,C] (values 0..255; C = the loaded model's channels,
 * mmla_od_image: 3, or 1 for a one-channel model) -> probs [n,K], K = mmla_od_classes (model.predict,
 * record_on_pc.py:159). */
int mmla_od_forward(mmla_ctx* ctx, const float* x_nhwc, int64_t n, float* probs, uint32_t flags);
/* Same on the uint8 image produced by mmla_od_features: [n,128,151,C]; a one-channel model reads channel 0
 * of the MMLA_OD_IMG_GRAY image. */
int mmla_od_forward_u8(mmla_ctx* ctx, const uint8_t* img, int64_t n, float* probs, uint32_t flags);

/* SI-NET predict on [n,256,39] -> probs [n,K] (SI record_on_pc.py:136;
 * speaker_identification_post_processing.py:272). */
int mmla_si_forward(mmla_ctx* ctx, const float* x, int64_t n, float* probs, uint32_t flags);

/* SI-NET up to the Bidirectional LSTM output (base_model.layers[-2].output,
 * speaker_identification.py:403): x [n,256,39] f32 -> emb [n,512] f32.  Host or device pointers;
 * micro-batching and the range guard as in mmla_si_forward (a host-pointer micro-batch that leaves the
 * fp16 range re-runs in exact f32, a device-pointer call flags it).  Needs SI weights; the loaded head
 * (K, softmax or sigmoid) does not enter the result: the Dense and head launches are skipped. */
int mmla_si_embed(mmla_ctx* ctx, const float* x, int64_t n, float* emb, uint32_t flags);

/*
 * Speaker registration, stage 1 of transfer_learning (speaker_identification.py:407-432): fit
 * Dense(n_classes, sigmoid) on frozen-base embeddings with categorical_crossentropy and RMSprop, as one
 * kernel launch (si_train.hip): restart r is one workgroup that runs all epochs x ceil(n_train / batch)
 * steps with the head and the optimiser state on chip.  Float32 arithmetic, Keras 2.6 semantics:
 *   forward  z = e W + b, s = 1 / (1 + exp(-z))
 *   loss     p = s / sum_k s_k, -log(clip(p_c, 1e-7, 1 - 1e-7)), mean over the batch (the last batch of
 *            an epoch is short when n_train % batch != 0)
 *   gradient dz_k = s_k (1 - s_k) (1 / S - [k = c] / s_c) / B, zero for a sample whose p_c is outside
 *            the clip range; gW = E^T dz, gb = sum dz
 *   RMSprop  rho 0.9, momentum 0, epsilon 1e-7 outside the root, accumulators from 0
 *   history  [R, epochs, 4] = loss, acc (each batch with the weights before its update), val_loss,
 *            val_acc (weights at the end of the epoch; NaN when n_val == 0); acc = first-index argmax
 * (stated from Keras' published source; TensorFlow is not available here: parity with TF unpinned).
 * emb [n_train,512], labels [n_train] in [0, n_classes); val_* [n_val] (n_val may be 0, pointers then
 * unused); w0 [R,512,K], b0 [R,K] initial head of each restart; perm [R,epochs,n_train] the sample
 * order of every epoch; w [R,512,K], b [R,K] the trained heads; history nullable.  Bit-reproducible,
 * and restart r's result does not depend on n_restarts.  MMLA_E_INVALID: n_classes outside
 * [1, MMLA_SI_TRAIN_MAX_CLASSES], batch < 1, n_train < 1, n_val < 0, n_restarts < 1, epochs < 0, and in
 * host-pointer calls a label outside [0, K) or a perm row that is not a permutation -- with device
 * pointers the caller guarantees both (the kernel only clamps a perm entry into [0, n_train), so a
 * broken contract gives a wrong fit, not a read outside emb).
 */
int mmla_si_head_fit(mmla_ctx* ctx, const float* emb, const int32_t* labels, int64_t n_train,
                     const float* val_emb, const int32_t* val_labels, int64_t n_val,
                     int32_t n_classes, int32_t n_restarts, int32_t epochs, int32_t batch, float lr,
                     const float* w0, const float* b0, const int32_t* perm, float* w, float* b,
                     float* history, uint32_t flags);

/*
 * Speaker registration, stage 2 of transfer_learning (speaker_identification.py:438-454): the whole
 * network trainable under a fresh RMSprop (the reference: lr 1e-6, 20 epochs, batch 8).  Float32 HIP
 * (si_bwd.hip), stated from the script and Keras 2.6's published source; TensorFlow is not available
 * here: parity with TF itself is unpinned.
 *   graph     SI-NET with the sigmoid head.  BatchNorm runs with its moving statistics, eps 1e-3 (the
 *             base is called with training=False, :406, which stays in force after trainable = True);
 *             Dropout is the identity; max-pool 'same' (T = 256 / 128 / 64: no pad occurs); Conv1D
 *             padding for k = 4 is 1 before, 2 after.
 *   trainable every Conv1D kernel and bias, every BN gamma and beta, the LSTM kernel, recurrent_kernel
 *             and bias of both directions, the head.  moving_mean / moving_variance are not: they come
 *             out bit-equal and their slots of a gradient are 0.
 *   loss      of a batch of B windows: mean_b[-log(clip(s_c / sum_k s_k, 1e-7, 1 - 1e-7))] + R, with
 *             R = 0.1 sum w^2 over the kernels of layer_with_weights-20, 22, 24, 26 + 0.2 sum w^2 over
 *             those of layer_with_weights-33, 35, 37, 39 (kernel_regularizer=l2, :175-206; kernels
 *             only).  The data term and its gradient at the logits are those of mmla_si_head_fit (zero
 *             for a sample whose p_c is outside the clip range); R is not divided by B, its gradient
 *             is 2 lambda w.
 *   optimiser the update of mmla_si_head_fit (rho 0.9, eps 1e-7 outside the root, momentum 0), every
 *             accumulator from 0, the head's included; the last batch of an epoch may be short.
 *   history   [epochs, 4] = loss (data + R, each batch with the weights before its update, sample-
 *             weighted mean), acc (first-index argmax), val_loss (data + R), val_acc with the weights
 *             at the end of the epoch; the val columns are NaN when n_val == 0.
 * Every sum has a fixed order and nothing is accumulated with atomics: the same inputs give the same
 * bits.  A step is a fixed sequence of launches on the context's stream without host synchronisation.
 * Both entries work on a copy of `packed` (weights.si_spec(n_classes) order, n_floats floats) and do not
 * touch the context's loaded model; host or device pointers.
 *
 * mmla_si_loss_grad: x [n,256,39], labels [n], n in [1, 4096] as ONE batch -> loss[0] the data term,
 *   loss[1] R; grad [n_floats] in the packed order.
 * mmla_si_finetune: x / labels [n_train], val_x / val_labels [n_val] (n_val may be 0, pointers then
 *   unused), perm [epochs, n_train] the sample order of every epoch -> packed_out [n_floats] (may be
 *   `packed`), history [epochs, 4].  epochs == 0 returns the input blob.  min(batch, n_train) <= 4096.
 * MMLA_E_INVALID, before any device work: n_classes outside [1, MMLA_SI_TRAIN_MAX_CLASSES], n_floats
 * that is not the blob's size for that head, batch < 1, n_train < 1 (n < 1), n_val < 0, epochs < 0, a
 * null pointer, and in host-pointer calls a label outside [0, K) or a perm row that is not a
 * permutation (device pointers: the caller guarantees both; a perm entry is clamped into the set and a
 * label only selects a lane, so a broken contract gives a wrong fit, not an access outside a buffer).
 */
int mmla_si_loss_grad(mmla_ctx* ctx, const float* packed, int64_t n_floats, int32_t n_classes,
                      const float* x, const int32_t* labels, int64_t n, float* loss, float* grad,
                      uint32_t flags);
int mmla_si_finetune(mmla_ctx* ctx, const float* packed, int64_t n_floats, int32_t n_classes,
                     const float* x, const int32_t* labels, int64_t n_train, const float* val_x,
                     const int32_t* val_labels, int64_t n_val, int32_t epochs, int32_t batch, float lr,
                     const int32_t* perm, float* packed_out, float* history, uint32_t flags);

/*
 * Training the SI base model from scratch: the reference's train(x_train, y_train, x_validate, y_validate)
 * (speaker_identification.py:221-250, driven by the __main__ at :506-555) on res_model's graph (:115-219).
 * Float32 HIP: si_bwd.hip's convolutions, pools, BiLSTM, L2 terms and RMSprop, and si_base.hip for what
 * separates training from fine-tuning.  Stated from the script and Keras 2.6's published source;
 * TensorFlow is not available here: parity with TF itself is unpinned, in particular for the three
 * statements marked (*).
 *   graph     as mmla_si_finetune above, with Dropout(0.25) on the [32, 128] map in front of
 *             AveragePooling1D(4), Dropout(0.2) on the 512-wide BiLSTM output, and a softmax head
 *             Dense(512 -> K), K <= MMLA_SI_BASE_MAX_CLASSES.
 *   training  Keras runs the network with training=True.  BatchNorm: per channel over the B T positions,
 *             the mean, then the biased variance of the centred values (two passes), eps 1e-3; after every
 *             step moving <- 0.99 moving + 0.01 batch, with that same BIASED variance (*): a rank-3
 *             input takes Keras's non-fused path (nn.moments, then _assign_moving_average of the variance
 *             it normalised with), unlike OD-NET's rank-4 inputs below.  Validation passes run in inference
 *             mode: moving statistics, no dropout.
 *   dropout   no mask is passed in.  Keep-bits are words of Philox4x32-10 with key = (low, high half of
 *             drop_seed's 64 bits; any int64_t value is a seed), counter = (element / 4, sample id, epoch, site), word = element % 4; site 0 is
 *             the [32, 128] map (element = 128 t + channel), site 1 the embedding.  The sample id is the
 *             row of the training set (sample_ids[i], or i), not the slot in the batch.  An element is kept
 *             iff its word >= 0x40000000 (site 0) or 0x33333333 (site 1), and kept values are scaled by
 *             float32(1 / 0.75) and float32(1 / 0.8).  TensorFlow's own generator is not reproduced.
 *   loss      of a batch of B windows: mean_b[logsumexp(z_b) - z_b[label]] + R, no clip (*): a Keras 2.6
 *             softmax output carries _keras_logits and categorical_crossentropy takes the logits path.
 *             dz = (softmax - onehot) / B.  R and its gradient as in mmla_si_finetune.  A hit is counted
 *             when the first maximum of z is the label.
 *   optimiser RMSprop as in mmla_si_finetune, every accumulator from 0; trainable is everything but
 *             moving_mean / moving_variance, whose gradient slots are 0 and which only the update above moves.
 *             Conv1D biases: every Conv1D output reaches the loss only through batch-statistics BNs, which
 *             cancel a per-channel constant, so their gradient is identically zero.  Their slots are
 *             reported as exactly 0 and they come out bit-equal; float32 Keras sums rounding noise there,
 *             which RMSprop turns into steps of up to 3.16 lr.
 *   callbacks EarlyStopping(val_loss, patience): the fit ends after the epoch in which val_loss has failed
 *             `patience` times in a row to go below its best; no restore_best_weights.
 *             ModelCheckpoint(val_categorical_accuracy, save_best_only, mode 'max', period): at every
 *             ckpt_period-th epoch whose val_categorical_accuracy is strictly above the best saved so far,
 *             the weights are copied on the device to best_out and best_epoch (0-based) is set.  Each is
 *             off when its argument is 0 or n_val == 0; while either is on, one history row is read back
 *             per epoch, otherwise a fit has no host synchronisation.
 *   history   [epochs, 4] = loss, categorical_accuracy (training mode, each batch with the weights before
 *             its update, sample-weighted), val_loss, val_categorical_accuracy (NaN when n_val == 0); rows
 *             after an early stop are NaN.
 * (*) the third: the initial state (weights.initial in the Python package) draws with numpy, not with
 * TensorFlow's generator.
 * Every sum has a fixed order and nothing is accumulated with atomics: the same inputs give the same bits.
 * Both training entries work on a copy of `packed` (weights.si_spec(n_classes) order) in the fine-tune's
 * workspace slot and do not touch the context's loaded model.  Host or device pointers (flags), epochs_run
 * and best_epoch included.
 *
 * mmla_si_base_drop_mask: the keep-bits of n samples as bytes, mask_a [n, 32, 128], mask_b [n, 512];
 *   sample_ids [n] nullable (= 0..n-1); n in [1, 2^20].
 * mmla_si_base_loss_grad: ONE training-mode batch, n in [1, 4096] -> loss[0] the data term, loss[1] R,
 *   grad [n_floats], moving_out [n_floats] (nullable): the blob with only the moving statistics advanced
 *   one step.
 * mmla_si_base_train: perm [epochs, n_train] -> packed_out [n_floats] the final state (may be `packed`),
 *   best_out [n_floats] (needed when ckpt_period > 0 and n_val > 0; written only when best_epoch >= 0),
 *   history [epochs, 4], epochs_run [1], best_epoch [1] (-1 if none).  epochs == 0 returns the input blob.
 * MMLA_E_INVALID, before any device work: n_classes outside [1, MMLA_SI_BASE_MAX_CLASSES], n_floats that is
 * not the blob's size for that head, batch < 1, n_train < 1 (n outside its range), n_val < 0, epochs < 0,
 * epoch < 0, patience < 0, ckpt_period < 0, lr negative or not finite, a null pointer, and in host-pointer
 * calls a label outside [0, K), a perm row that is not a permutation or a sample id < 0 (device pointers: a
 * perm entry is clamped into the set, a label is clamped into [0, K), a sample id is only a counter word,
 * so a broken contract gives a wrong fit, not an access outside a buffer).
 */
#define MMLA_SI_BASE_MAX_CLASSES 1024
int mmla_si_base_drop_mask(mmla_ctx* ctx, int64_t drop_seed, int32_t epoch, const int32_t* sample_ids,
                           int64_t n, uint8_t* mask_a, uint8_t* mask_b, uint32_t flags);
int mmla_si_base_loss_grad(mmla_ctx* ctx, const float* packed, int64_t n_floats, int32_t n_classes,
                           const float* x, const int32_t* labels, int64_t n, int64_t drop_seed,
                           int32_t epoch, const int32_t* sample_ids, float* loss, float* grad,
                           float* moving_out, uint32_t flags);
int mmla_si_base_train(mmla_ctx* ctx, const float* packed, int64_t n_floats, int32_t n_classes,
                       const float* x, const int32_t* labels, int64_t n_train, const float* val_x,
                       const int32_t* val_labels, int64_t n_val, int32_t epochs, int32_t batch, float lr,
                       const int32_t* perm, int64_t drop_seed, int32_t patience, int32_t ckpt_period,
                       float* packed_out, float* best_out, float* history, int32_t* epochs_run,
                       int32_t* best_epoch, uint32_t flags);

/*
 * Adapting OD-NET to a room: OverlapDetector.continue_train_model (overlap_detector.py:480-509), the
 * trained detector fitted further on labelled feature images.  Float32 HIP (od_bwd.hip, with conv.hip's
 * exact-f32 MFMA convolution and si_bwd.hip's BiLSTM), stated from the script and Keras 2.6's published
 * source; TensorFlow is not available here: parity with TF itself is unpinned.
 *   graph     OD-NET (oracle/nets_torch.Nets.od_forward): img_u8 [n, h, w, C] PNG values taken as float, C
 *             the channels of the blob's stem kernel [1,1,C,16]: 3, or 1 for a blob 32 floats shorter (the
 *             network of OverlapDetector(imagetype='gray'); n_floats tells (K, C), the gradient and every
 *             blob going out have the blob's own layout: 16 stem-kernel entries for C = 1);
 *             stem Conv2D 1x1; nine res blocks BN - ELU - Conv 3x3 - BN - ELU - Conv (4,1) with pool =
 *             (T,F,F,T,F,F,T,F,F): a pool block adds MaxPool2D(2,'same') of the main path to a 1x1
 *             stride-2 shortcut.  Conv 'same': the (4,1) kernel pads 1 above, 2 below; the pool pads odd
 *             sizes with -inf (ties go to the first candidate in row-major order).  Mean over H, a BiLSTM
 *             over the ceil(w / 8) columns (D 128, U 256, the backward direction over the reversed
 *             sequence), Dropout(0.25), LeakyReLU(float32(0.3)), Dense(K), softmax.  h in [8, 128], w in
 *             [8, 151]: 1..19 LSTM steps.
 *   training  BatchNorm on batch statistics: per channel over n h w, mean and biased variance, eps 1e-3;
 *             after every step moving <- 0.99 moving + 0.01 batch, the variance Bessel-corrected (x N /
 *             max(N - 1, 1): rank-4 inputs take Keras's fused path).  Dropout: x * float32(1 / 0.75) *
 *             keep, keep = drop_mask != 0, an input drawn on the host (no RNG runs on the device); a null
 *             drop_mask keeps every unit (the scale stays).  Validation passes run in inference mode:
 *             moving statistics, no dropout, no scale.
 *   loss      weighted_categorical_crossentropy (:62-79): p <- p / sum p, clip(p, 1e-7, 1 - 1e-7), sample
 *             loss -class_w[c] log p_c, batch mean.  A sample clipped at either end contributes zero
 *             gradient.  No L2 term (ResLSTM builds every block with regularized=0).
 *   optimiser Keras Adadelta, rho 0.95, eps 1e-7: a <- rho a + (1 - rho) g^2; u = sqrt(d + eps) /
 *             sqrt(a + eps) g; v <- v - lr u; d <- rho d + (1 - rho) u^2; every accumulator from 0 (a
 *             checkpoint's optimizer slots are not read).  lr [epochs] is constant within an epoch.
 *             Trainable: every kernel, bias, gamma, beta, the LSTM tensors, the head.  moving_mean /
 *             moving_variance are not: their gradient slots are 0 and only the update above moves them.
 *   stopping  EarlyStopping(monitor='val_loss', patience) without restore_best_weights: the fit ends after
 *             the first epoch whose val_loss has not improved on the best for `patience` epochs; the last
 *             epoch's weights are returned.  patience == 0 or n_val == 0 turns it off.  It costs one
 *             history-row read-back per epoch; with it off a fit has no host synchronisation.
 *             ModelCheckpoint is not mirrored.
 *   history   [epochs, 5] = loss (each batch in training mode with the weights before its update, sample-
 *             weighted mean), acc (first-index argmax), val_loss, val_acc (NaN when n_val == 0), lr.  Rows
 *             after an early stop are NaN.
 * Every sum has a fixed order and nothing is accumulated with atomics: the same inputs give the same bits.
 * Both entries work on a copy of `packed` (weights.od_spec(K) order, n_floats floats) in a workspace slot of
 * their own and do not touch the context's loaded model.  packed, the images, labels, perm, drop_mask and
 * every output are host or device pointers (flags); class_w [K] and lr [epochs] are always host pointers.
 * K, the classes of the head, is read from n_floats = (the blob below the head) + 513 K, 2 <= K <=
 * MMLA_OD_MAX_CLASSES: class_w is [K], labels lie in [0, K), the workspace pieces for the softmax outputs,
 * the logit gradients and the head's gradients are sized by K.  The logits are z_k = b_k then fmaf over the
 * 512 inputs ascending; q = p / sum p with k ascending; the gradient at the logits is class_w[c] (q_k -
 * [k = c]) / batch inside the clip range, else 0 for the whole row; a hit is the first-index argmax of q.
 * A fit at K = 2 gives the bits it gave before K was a parameter.
 *
 * mmla_od_loss_grad: ONE training-mode batch of n <= MMLA_OD_TRAIN_MAX_BATCH images, drop_mask [n, 512]
 *   (nullable) -> loss [1], grad [n_floats] in the packed order, moving_out [n_floats] (nullable): the
 *   blob with only the moving statistics advanced one step.
 * mmla_od_finetune: img_u8 / labels [n_train], val_img / val_labels [n_val] (n_val may be 0, pointers then
 *   unused), perm [epochs, n_train] the sample order of every epoch, drop_mask [epochs, n_train, 512]
 *   indexed by sample (nullable) -> packed_out [n_floats] (may be `packed`), history [epochs, 5],
 *   epochs_run [1].  epochs == 0 returns the input blob.
 * MMLA_E_INVALID, before any device work: n_floats that is no K's OD blob size, h or w outside the
 * range, batch < 1, min(batch, n_train) > MMLA_OD_TRAIN_MAX_BATCH (n outside [1, MAX_BATCH]), n_train < 1,
 * n_val < 0, epochs < 0, patience < 0, a null pointer, a class_w or lr that is negative or not finite, and
 * in host-pointer calls a label outside [0, K) or a perm row that is not a permutation (device pointers:
 * a perm entry is clamped into the set, a label selects a lane by its lowest bit at K = 2 and is clamped
 * into [0, K - 1] at K > 2, a mask byte is read as zero / non-zero, so a broken contract gives a wrong fit,
 * not an access outside a buffer).
 */
#define MMLA_OD_TRAIN_MAX_BATCH 64
int mmla_od_loss_grad(mmla_ctx* ctx, const float* packed, int64_t n_floats, const uint8_t* img_u8,
                      const int32_t* labels, int64_t n, int32_t h, int32_t w, const float* class_w,
                      const uint8_t* drop_mask, float* loss, float* grad, float* moving_out,
                      uint32_t flags);
int mmla_od_finetune(mmla_ctx* ctx, const float* packed, int64_t n_floats, const uint8_t* img_u8,
                     const int32_t* labels, int64_t n_train, const uint8_t* val_img,
                     const int32_t* val_labels, int64_t n_val, int32_t h, int32_t w, const float* class_w,
                     int32_t epochs, int32_t batch, const float* lr, const int32_t* perm,
                     const uint8_t* drop_mask, int32_t patience, float* packed_out, float* history,
                     int32_t* epochs_run, uint32_t flags);

/*
 * Training OD-NET from scratch: OverlapDetector.train_model (overlap_detector.py:392-451) with its class
 * balancing augment_images (:198-220) and its tf.keras.metrics.AUC() (:403).  The fit is mmla_od_finetune's
 * statement above in every respect -- graph, BatchNorm rules, loss, Adadelta, validation mode, argument
 * checks, the epochs == 0 identity, no host synchronisation unless a callback is live -- on the same engine
 * and the same driver, with three differences:
 *   dropout   no host mask: drop_seed keys Philox4x32-10 (Salmon et al., SC'11) on the device, the generator
 *             of mmla_si_base_train at a site of its own.  Key = the two halves of drop_seed, counter =
 *             (element / 4, sample id, epoch, 2), word = element % 4 over the 512 embedding elements; an
 *             element is kept iff its word >= 0x40000000.  The sample id is the row of the training set, not
 *             the slot in the batch.  mmla_od_drop_mask writes the same bits as bytes: fed to
 *             mmla_od_finetune they give the same fit, bit for bit.
 *   callbacks EarlyStopping(val_loss, patience) as above and ModelCheckpoint(val_categorical_accuracy,
 *             save_best_only, mode 'max', period = ckpt_period) as mmla_si_base_train states it: best_out
 *             [n_floats] (needed when ckpt_period > 0 and n_val > 0; written only when best_epoch >= 0),
 *             best_epoch [1] (-1 if none).  restore_best_weights is not mirrored (the script never sets it).
 *   history   [epochs, 7] = loss, acc, val_loss, val_acc, lr, auc, val_auc.  auc: the counts accumulate over
 *             the batches of the epoch from the training-mode softmax outputs (each batch with the weights
 *             before its update), as Keras accumulates a metric during fit; val_auc over the validation
 *             passes, NaN when n_val == 0.  Rows after an early stop are NaN.
 *
 * AUC (mmla_od_auc, and the two history columns): tf.keras.metrics.AUC() at its defaults, stated from Keras
 * 2.6's published source (parity with TF itself is unpinned).  200 float32 thresholds: float32(0 - 1e-7),
 * float32((i + 1) / 199.0) for i = 0..197 with the quotient in double, float32(1 + 1e-7).  multi_label =
 * False: all K n entries of probs [n, K] are binary predictions against the entries of the one-hot label
 * rows; a prediction is positive iff p > thr, strictly.  Per threshold TP (the label's entry) and FP (the
 * K - 1 others) are integers (one thread per threshold walks the rows: no atomics); recall = TP / n, fpr =
 * FP / ((K - 1) n), 0 where a denominator is 0; auc = sum_{t=0}^{198} (fpr[t] - fpr[t+1]) (recall[t] +
 * recall[t+1]) / 2.  Deliberate
 * deviation: the formula is evaluated in double from the integer counts and rounded to float32 once, where
 * Keras sums in float32 -- a difference of at most about 200 x 2^-24.
 *
 * mmla_od_augment: the pyramid blur.  out[k] [h, w, 3] = img[src[k]] after levels[k] rounds of cv.pyrDown
 * then cv.pyrUp, cropped once at the end with [:, :-1]; level 0 is a copy.  Stated from OpenCV's published
 * uint8 pyramid code; OpenCV is not available here: parity with OpenCV unpinned.  Each channel alone, exact
 * integer arithmetic, k = (1, 4, 6, 4, 1):
 *   pyrDown [H, W] -> [(H+1)/2, (W+1)/2]: d[y,x] = (sum_{i,j=-2..2} k[i] k[j] s[r(2y+i), r(2x+j)] + 128) >> 8,
 *           r = BORDER_REFLECT_101 (-1 -> 1, -2 -> 2, N -> N-2, N+1 -> N-3)
 *   pyrUp   [H, W] -> [2H, 2W]: along a row e[2x] = s[x-1] + 6 s[x] + s[x+1], e[2x+1] = 4 (s[x] + s[x+1]), then
 *           the same rule down the columns of e, result (v + 32) >> 6; s[-1] = s[1], s[N] = s[N-1] on both axes
 *   levels  the first pyrUp of a w-wide image is w + 1 wide; that column stays in the working image through
 *           every further level (later pyrDowns read it) and is cropped once, after the last
 * h even in [8, 128], w odd in [9, 151] (other sizes would change the reference's output shape); n in
 * [1, 2^24], m in [0, 2^24]; a level in [0, MMLA_OD_AUG_MAX_LEVELS].
 *
 * mmla_od_drop_mask: mask [n, 512] bytes (1 kept), sample_ids [n] nullable (= 0..n-1), n in [1, 2^20].
 * mmla_od_auc: probs [n, 2], labels [n] in {0, 1}, n in [1, 2^24] -> auc_out [1].
 * mmla_od_auc_k: probs [n, n_classes], labels [n] in [0, n_classes), 2 <= n_classes <= MMLA_OD_MAX_CLASSES;
 *   at 2 it is mmla_od_auc, bit for bit.
 * Host or device pointers (flags) throughout; class_w and lr are host pointers as above.
 * MMLA_E_INVALID, before any device work: what mmla_od_finetune rejects, ckpt_period < 0, epoch < 0, a size or
 * count or n_classes outside the ranges above, a null pointer, and in host-pointer calls a src outside [0, n),
 * a level outside its range, a label outside [0, K) or a sample id < 0 (device pointers: src and levels are
 * clamped into range, a label selects a lane by its lowest bit (K = 2) or is clamped (K > 2), a sample id is
 * only a counter word, so a broken
 * contract gives a wrong result, not an access outside a buffer).
 */
#define MMLA_OD_AUG_MAX_LEVELS 8
int mmla_od_augment(mmla_ctx* ctx, const uint8_t* img, int64_t n, int32_t h, int32_t w, const int32_t* src,
                    const int32_t* levels, int64_t m, uint8_t* out, uint32_t flags);
int mmla_od_auc(mmla_ctx* ctx, const float* probs, const int32_t* labels, int64_t n, float* auc_out,
                uint32_t flags);
int mmla_od_auc_k(mmla_ctx* ctx, const float* probs, const int32_t* labels, int64_t n, int32_t n_classes,
                  float* auc_out, uint32_t flags);
int mmla_od_drop_mask(mmla_ctx* ctx, int64_t drop_seed, int32_t epoch, const int32_t* sample_ids, int64_t n,
                      uint8_t* mask, uint32_t flags);
int mmla_od_train(mmla_ctx* ctx, const float* packed, int64_t n_floats, const uint8_t* img_u8,
                  const int32_t* labels, int64_t n_train, const uint8_t* val_img, const int32_t* val_labels,
                  int64_t n_val, int32_t h, int32_t w, const float* class_w, int32_t epochs, int32_t batch,
                  const float* lr, const int32_t* perm, int64_t drop_seed, int32_t patience,
                  int32_t ckpt_period, float* packed_out, float* best_out, float* history,
                  int32_t* epochs_run, int32_t* best_epoch, uint32_t flags);

/* Fused WAV->class pipelines (no PNG, no host round trip): probs [n,K] f32 (nullable),
 * argmax [n] i32 (nullable; -1 for 'silent' clips), silent [n] u8 (nullable).  'silent' = fewer
 * than 4000 samples (lens[c], or clip_len without lens): OD record_on_pc.py:141-154 logs it and
 * skips predict, SI speaker_identification.py:375-376 returns the 'silent' sentinel; their probs
 * are still computed (on the zero-padded clip) but carry no meaning. */
int mmla_od_pipeline(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                     const int32_t* lens, int32_t clip_len, float* probs, int32_t* argmax,
                     uint8_t* silent, uint32_t flags);
int mmla_si_pipeline(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                     const int32_t* lens, int32_t clip_len, float* probs, int32_t* argmax,
                     uint8_t* silent, uint32_t flags);

/*
 * Mean structural similarity of n pairs of uint8 images a, b [n,h,w,c] -> out [n] f32: replaces
 * skimage.metrics.structural_similarity(image1, image2, multichannel=True) of compare_images
 * (OverlapDetection/scripts/record_on_pi.py:39-48) with scikit-image's defaults for uint8 input: uniform
 * 7 x 7 window, K1 0.01, K2 0.03, data_range 255, sample covariance, the SSIM map cropped by 3 pixels
 * on every side, the mean over the cropped map per channel and then over channels.  The window sums are
 * exact integers, the rest is float32 (within 2e-6 of float64); two equal images give exactly 1.  A
 * pair's result is bit-identical wherever it sits in the batch (fixed-order reduction, no atomics).
 * (Stated from scikit-image's published source; the library is not available here: parity with it is
 * unpinned.)  MMLA_E_INVALID for h or w < 7 or c not in {1, 3, 4}.
 */
int mmla_ssim_u8(mmla_ctx* ctx, const uint8_t* a, const uint8_t* b, int64_t n, int32_t h, int32_t w,
                 int32_t c, float* out, uint32_t flags);

/*
 * mmla_od_pipeline with the denoise-and-compare silence gate of the edge loop
 * (OverlapDetection/scripts/record_on_pi.py:103-124).  Per clip:
 *   image A = the front-end on the raw PCM;
 *   y = pcm / 32768, then nr_passes times (the reference: NOISE_REDUCE_TIMES = 4): the stationary gate
 *     of mmla_nr_reduce on the clip's first min(clip_len, 24000) samples, written as PCM_16 (mmla_pcm16's
 *     rule) and read back (/ 32768).  With lens the clip is denoised zero-extended to that length and
 *     the samples from lens[c] on are zeroed after every pass;
 *   image B = the front-end on the denoised int16 PCM;  ssim[c] = SSIM(A, B) (mmla_ssim_u8);
 *   silent[c] = fewer than 4000 samples OR ssim[c] < ssim_threshold (the reference: 0.3);
 *   probs[c] = OD-NET on image B;  argmax[c] = -1 where silent.
 * nr_passes = 0: B = A, ssim = 1, the results of mmla_od_pipeline, no noise profile needed.
 * MMLA_E_INVALID: nr_passes < 0, or nr_passes > 0 before mmla_nr_set_noise.  ssim [n] f32 is nullable.
 * The gate's SSIM is defined on the ZCR images (record_on_pi.py:117-120): with a loaded model whose image
 * type (mmla_od_set_image_type) is not MMLA_OD_IMG_ZCR this call is MMLA_E_INVALID.
 * Micro-batched as mmla_od_pipeline (mmla_set_microbatch lists the extra workspace).  The gate runs at
 * most 512 clips per launch with a stream synchronisation between launches and between passes, so with
 * MMLA_DEVICE_PTR and nr_passes > 0 this call synchronises the context stream internally (its last
 * launches are still only enqueued).
 */
int mmla_od_pipeline_gated(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                           const int32_t* lens, int32_t clip_len, int32_t nr_passes,
                           float ssim_threshold, float* probs, int32_t* argmax, uint8_t* silent,
                           float* ssim, uint32_t flags);

/*
 * Stationary spectral-gate noise reduction, replaces nr.reduce_noise(y_noise=noise, y=y, sr=sr,
 * stationary=True) (OverlapDetection/scripts/record_on_pc.py:208-212,
 * SpeakerIdentification/scripts/record_on_pc.py:189, speaker_identification_post_processing.py:171)
 * with noisereduce 2.0.x defaults (n_fft 1024, hop 256, n_std 1.5, 500 Hz x 50 ms mask smoothing,
 * chunk_size 600000, padding 30000).  sr must be 16000.
 * mmla_nr_set_noise: noise [n_noise] f32 (librosa.load output; the first chunk_size samples are
 * used) -> per-bin threshold kept in the context.
 * mmla_nr_reduce: y [n_signals, stride] f32, each signal `len` samples -> out [n_signals, len] f32;
 * signals longer than chunk_size are gated chunk by chunk with `padding` samples of context.
 */
int mmla_nr_set_noise(mmla_ctx* ctx, const float* noise, int64_t n_noise, int32_t sr,
                      uint32_t flags);
int mmla_nr_reduce(mmla_ctx* ctx, const float* y, int64_t n_signals, int64_t stride, int64_t len,
                   float* out, uint32_t flags);

/*
 * Silence removal, replaces save_wave_file(silence_remove=True) (OverlapDetection/scripts/
 * record_on_pc.py:214-226, frame_generator :229-243, vad_collector :246-295; the same functions in
 * SpeakerIdentification/scripts/record_on_pc.py:196 and speaker_identification_post_processing.py:
 * 176-187,225-251).  Frames of 30 ms (480 samples) that END BEFORE the item's last sample,
 * webrtcvad.Vad(mode).is_speech per frame (py-webrtcvad / WebRTC fixed-point VAD, 16 kHz path),
 * the 10-frame ring-buffer trigger (> 90 % voiced / unvoiced), and the voiced frames written back
 * in order: item i -> out + i * stride, out_lens[i] samples (a multiple of 480).
 * mmla_vad_reset: (re)creates n_streams independent detectors in the context.  The reference keeps
 * ONE module-level Vad(3) whose GMM state carries across clips; a stream is that object: its items
 * are processed in order, and its state persists across calls until the next reset.
 * mmla_vad_remove_silence: n_items = n_streams * items_per_stream; stream s owns items
 * [s * items_per_stream, (s + 1) * items_per_stream).  speech [n_items][max_frames] u8 receives the
 * per-frame decisions (nullable); max_frames 0 = the frames of the widest item.
 * mmla_vad_collect: the collector and rewrite alone, on caller-supplied decisions `speech`.
 * mmla_pcm16: sf.write(path, y, 16000) of float audio as PCM_16 (:212): (short) lrintf(y * 32767).
 */
int mmla_vad_reset(mmla_ctx* ctx, int64_t n_streams, int32_t mode);
int mmla_vad_remove_silence(mmla_ctx* ctx, const int16_t* pcm, int64_t n_items, int64_t stride,
                            const int32_t* lens, int32_t clip_len, int64_t items_per_stream,
                            int16_t* out, int32_t* out_lens, uint8_t* speech, int32_t max_frames,
                            uint32_t flags);
int mmla_vad_collect(mmla_ctx* ctx, const int16_t* pcm, int64_t n_items, int64_t stride,
                     const int32_t* lens, int32_t clip_len, const uint8_t* speech, int32_t max_frames,
                     int16_t* out, int32_t* out_lens, uint32_t flags);
int mmla_pcm16(mmla_ctx* ctx, const float* y, int64_t n, int16_t* out, uint32_t flags);

/*
 * A bank of noise profiles: one per microphone of a room served by one context (each microphone
 * records its own ambient noise at start-up: recording(..., noise_reduced=False) -> NOISE_PATH,
 * OverlapDetection/scripts/record_on_pc.py:133).
 * mmla_nr_set_noise_bank: profile p = noise + p * stride, its first lens[p] samples (lens nullable:
 *   len; 2 <= lens[p] <= len, host pointers: checked, device pointers: clamped by the kernels) ->
 *   thresholds [n_profiles][513] kept in the context, replacing the bank it held.  All profiles come
 *   from one launch sequence with one stream synchronisation.  mmla_nr_set_noise is a bank of one.
 * mmla_nr_reduce_bank: mmla_nr_reduce with signal i gated against profile[i] (nullable: profile 0, the
 *   bits of mmla_nr_reduce).  Host pointers: a profile[i] outside [0, n_profiles) is MMLA_E_INVALID;
 *   device pointers cannot be checked, the kernels clamp the index into the bank (the convention of
 *   the VAD's lens).
 */
int mmla_nr_set_noise_bank(mmla_ctx* ctx, const float* noise, int64_t n_profiles, int64_t stride,
                           const int32_t* lens, int32_t len, int32_t sr, uint32_t flags);
int mmla_nr_reduce_bank(mmla_ctx* ctx, const float* y, int64_t n_signals, int64_t stride, int64_t len,
                        const int32_t* profile, float* out, uint32_t flags);

/*
 * Non-stationary spectral gate: noisereduce 2.0.x reduce_noise(y=y, sr=sr) in its default mode
 * (stationary=False, SpectralGateNonStationary), which needs NO noise recording.  The reference's
 * scripts never call this mode; it is here for rooms whose microphones have no ambient-noise clip or
 * whose noise changes during a session.  Parity with the library is unpinned (it is not installed);
 * the definition is the numpy / scipy restatement in tests/nr_ns_ref.py.  Per chunk buffer (chunks,
 * padding, STFT, the 33 x 7 mask smoothing, iSTFT and the kept interior are mmla_nr_reduce's):
 *   A = |STFT|;  t = time_constant_s * sr / 256;  b = (sqrt(1 + 4 t^2) - 1) / (2 t^2);
 *   smooth = scipy.signal.filtfilt([b], [1, b - 1], A, axis=time, padtype=None), evaluated per bin as
 *     the sequential recurrence  z = (1-b) A[0];  f[t] = b A[t] + z;  z = (1-b) f[t]  forward, then
 *     z = (1-b) f[T-1];  g[t] = b f[t] + z;  z = (1-b) g[t]  backward, in float64 without FMA;
 *   mask = 1 / (1 + exp(-((A - smooth) / smooth - thresh_n_mult) * sigmoid_slope)), smoothed 33 x 7,
 *   out = istft(STFT * mask), float32.
 * One deliberate deviation: where smooth == 0 the mask is 0.  That happens only for a buffer of nothing
 * but zeros, for which the library computes 0 / 0 and returns NaN; here such a buffer comes out as zeros.
 * mmla_nr_set_nonstationary: the gate's parameters, kept in the context, which starts with noisereduce's
 *   defaults (2.0 s, 2.0, 10.0, 16000): no call is needed for them.  MMLA_E_INVALID: time_constant_s or
 *   sigmoid_slope not finite or <= 0, thresh_n_mult not finite, an sr whose smoothing filter is not
 *   33 x 7 (15360..16000), or an sr that differs from that of a noise bank the context holds.
 * mmla_nr_reduce_ns: mmla_nr_reduce's contract (chunking, host / device pointers, at most 512 chunk
 *   buffers per launch) without a noise profile.
 * MMLA_NR_NONSTATIONARY in the flags of mmla_condition, mmla_{od,si,room}_pipeline_conditioned and
 *   mmla_od_pipeline_gated: the nr_passes passes run this gate with the context's parameters, `profile`
 *   is ignored and no noise bank is required; everything else (the PCM_16 round trip per pass, lens,
 *   micro-batching, re-runs, stream synchronisation) is unchanged.  Without the flag those calls behave
 *   as before, MMLA_E_INVALID for nr_passes > 0 without a bank included.
 * The smoothed floor sees the whole buffer: the zero padding and a clip's zero tail pull it down near
 * the ends, as the library's does for a buffer of that length.  So the fused calls' rule "gated
 * zero-extended to clip_len" is the definition here too: clip c's result is mmla_nr_reduce_ns of the
 * clip zero-extended to clip_len, NOT of the clip cut at lens[c].
 */
int mmla_nr_set_nonstationary(mmla_ctx* ctx, double time_constant_s, double thresh_n_mult,
                              double sigmoid_slope, int32_t sr);
int mmla_nr_reduce_ns(mmla_ctx* ctx, const float* y, int64_t n_signals, int64_t stride, int64_t len,
                      float* out, uint32_t flags);

/*
 * The PC loops' pre-conditioning of every recorded clip as one batched call: the batched
 * save_wave_file(noise_reduce=True, silence_remove=...) of OverlapDetection/scripts/record_on_pc.py:133,
 * 141-154,200-226, SpeakerIdentification/scripts/record_on_pc.py:117-134,178-205 and
 * SpeakerIdentification/scripts/record_on_pi.py:101-127,228-240.  Per clip c, over its whole length:
 *   y = pcm / 32768, then nr_passes times (the loops: 1; standardize_audio: 3) the stationary gate with
 *     noise profile profile[c] (nullable: profile 0) of the bank, written as PCM_16 (mmla_pcm16's rule)
 *     and read back.  With lens the clip is gated zero-extended to clip_len and the samples from lens[c]
 *     on are zeroed after every pass (mmla_od_pipeline_gated's rule);
 *   silence_remove != 0: mmla_vad_remove_silence on the int16 result with that call's stream layout --
 *     stream s owns clips [s * items_per_stream, (s + 1) * items_per_stream), in order, on the detector
 *     state mmla_vad_reset created, which persists across calls;
 *   kept_len[c] = the samples the rewritten file holds (a multiple of 480 after silence removal, else
 *     the clip's length); out_pcm [n_clips, clip_len] = those samples, then zeros.  Both nullable.
 * MMLA_E_INVALID: clip_len outside [1, 600000] (one gate chunk), clip_stride < clip_len, nr_passes < 0,
 * nr_passes > 0 without a noise bank, n_clips not a multiple of items_per_stream, silence_remove without
 * an mmla_vad_reset of n_clips / items_per_stream streams, a host profile[c] outside the bank (device
 * pointers: clamped by the kernels).
 * Micro-batched in whole streams (multiples of items_per_stream, at least one stream even where
 * mmla_set_microbatch asks for less); the detectors advance exactly once per clip whatever the
 * micro-batch size and whether a micro-batch had to be re-run (a range-guard or split-BiLSTM re-run
 * repeats the network alone on the conditioning already made; an allocation failure repeats the
 * micro-batch with fewer clips from the detectors' saved state).  The gate runs at most 512 clips per
 * launch with a stream synchronisation between launches and between passes, so with MMLA_DEVICE_PTR and
 * nr_passes > 0 these calls synchronise the context stream internally (their last launches are still
 * only enqueued).
 * mmla_{od,si}_pipeline_conditioned: the conditioning, then mmla_{od,si}_pipeline on the conditioned
 * clips with lens = kept_len: silent[c] = kept_len[c] < 4000 (record_on_pc.py:141-154), argmax -1 there.
 * nr_passes = 0 with silence_remove = 0 is mmla_{od,si}_pipeline bit for bit.
 */
int mmla_condition(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                   const int32_t* lens, int32_t clip_len, const int32_t* profile, int32_t nr_passes,
                   int32_t silence_remove, int64_t items_per_stream, int16_t* out_pcm,
                   int32_t* kept_len, uint32_t flags);
int mmla_od_pipeline_conditioned(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                                 const int32_t* lens, int32_t clip_len, const int32_t* profile,
                                 int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                                 int16_t* out_pcm, int32_t* kept_len, float* probs, int32_t* argmax,
                                 uint8_t* silent, uint32_t flags);
int mmla_si_pipeline_conditioned(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                                 const int32_t* lens, int32_t clip_len, const int32_t* profile,
                                 int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                                 int16_t* out_pcm, int32_t* kept_len, float* probs, int32_t* argmax,
                                 uint8_t* silent, uint32_t flags);

/*
 * Both detectors for a room: mmla_od_pipeline_conditioned and mmla_si_pipeline_conditioned on the same
 * clips from ONE conditioning, so the gate and the silence removal run once and every stream's detector
 * advances once per clip (two single calls on one context would advance it twice over the same audio).
 * Arguments, limits and MMLA_E_INVALID cases are mmla_condition's; MMLA_E_NOWEIGHTS names the model that
 * is not loaded (both must be, in this context).  Per micro-batch (whole streams, OD's micro-batch cap):
 * the conditioning, then the OD front-end + network, then the SI front-end + network on the same
 * conditioned clips with lens = kept_len.  silent[c] = kept_len[c] < 4000 is one array (both loops' rule);
 * od_argmax and si_argmax are -1 there.  od_probs [n_clips, 2], si_probs [n_clips, K].
 * Every output equals, byte for byte, what the two single calls return, each on a fresh context of its
 * own with the same bank, mmla_vad_reset and arguments, and the detector state left behind is that of one
 * of them: under host and device pointers, for any micro-batch size, and when a micro-batch is re-run
 * (a range-guard or split-BiLSTM re-run repeats that network alone on the conditioning already made; an
 * allocation failure repeats the micro-batch with fewer clips from the detectors' saved state).
 * nr_passes = 0 with silence_remove = 0 is mmla_od_pipeline plus mmla_si_pipeline, bit for bit.
 * Stream synchronisation under MMLA_DEVICE_PTR: as mmla_condition.
 */
int mmla_room_pipeline_conditioned(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                                   const int32_t* lens, int32_t clip_len, const int32_t* profile,
                                   int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                                   int16_t* out_pcm, int32_t* kept_len, float* od_probs,
                                   int32_t* od_argmax, float* si_probs, int32_t* si_argmax,
                                   uint8_t* silent, uint32_t flags);

/*
 * Overlap synthesis: layered mixes of int16 recordings, the overlay chain of generate_overlap_segment
 * (OverlapDetection/scripts/data_augmentation.py:20-34): pydub's AudioSegment.overlay(seg, position) with
 * times = 1 and no gain is audioop.add(canvas[pos : pos + n], seg[:n], 2), n = min(len(seg),
 * max(0, len(canvas) - pos)), every sum clamped to [-32768, 32767]; a chain of overlays applies that rule
 * in order, and the order matters because every step saturates.  Bit-identical to CPython's audioop.add
 * (pydub is not installed here: its slicing arithmetic is restated from its published source, parity
 * with the library itself is unpinned).
 *
 * All clips read one pool [pool_len] int16 (the recordings laid end to end).  Clip c has n_layers[c]
 * layers, 1 .. MMLA_MIX_MAX_LAYERS; the descriptor arrays src_off (int64 sample offset into the pool),
 * src_len and pos are [n_clips, MMLA_MIX_MAX_LAYERS], entries at or past n_layers[c] are not read.  Layer 0
 * is the canvas, at position 0 (pos[c][0] is not used).
 *   canvas_len = min(src_len[c][0], clip_len)
 *   s < canvas_len:  v = pool[off_0 + s]; then for l = 1 .. n_layers[c] - 1 in order, where
 *                    pos_l <= s < pos_l + min(len_l, canvas_len - pos_l):  v = clamp(v + pool[off_l + s - pos_l])
 *   canvas_len <= s < clip_len:  0
 * mmla_od_mix: out [n_clips, out_stride] int16, only [0, clip_len) of a row is written (out_stride >=
 *   clip_len, neither need be a multiple of anything); out_len [n_clips] = canvas_len (nullable).
 *   clip_len in [1, 600000].  Host or device pointers (MMLA_DEVICE_PTR: one launch, asynchronous).
 *   Host-pointer calls check the plan before any launch: MMLA_E_INVALID, with the clip and the layer in
 *   mmla_last_error, for a layer count outside 1..MMLA_MIX_MAX_LAYERS, a negative offset, length or
 *   position, or off + len > pool_len.  A device plan cannot be seen by the host: the kernel clips every
 *   layer to the pool and skips one with a negative offset, length or position, so a bad plan gives a
 *   wrong mix, never a read outside [0, pool_len).
 * mmla_od_pipeline_mixed: the mix at clip_len = MMLA_OD_CLIP fused in front of mmla_od_pipeline.  The
 *   pool and the plan are uploaded once per host-pointer call; per micro-batch (OD's size) the mix writes a
 *   workspace buffer that the front-end and OD-NET read with lens = out_len, so the mixed PCM never
 *   reaches the host.  silent[c] = canvas_len < 4000, argmax -1 there.  probs, argmax and silent are
 *   bit-identical to mmla_od_pipeline on the output of mmla_od_mix with lens = out_len.  MMLA_E_INVALID
 *   as mmla_od_mix, MMLA_E_NOWEIGHTS without OD weights; micro-batching, the range guard and its re-runs
 *   as the conditioned pipelines (a re-run repeats the network alone on the clips already mixed).
 *   Workspace per clip of a micro-batch: the mixed clip, 48 KB (mmla_set_microbatch).
 */
#define MMLA_MIX_MAX_LAYERS 8
int mmla_od_mix(mmla_ctx* ctx, const int16_t* pool, int64_t pool_len, int64_t n_clips, const int32_t* n_layers,
                const int64_t* src_off, const int32_t* src_len, const int32_t* pos, int32_t clip_len,
                int16_t* out, int64_t out_stride, int32_t* out_len, uint32_t flags);
int mmla_od_pipeline_mixed(mmla_ctx* ctx, const int16_t* pool, int64_t pool_len, int64_t n_clips,
                           const int32_t* n_layers, const int64_t* src_off, const int32_t* src_len,
                           const int32_t* pos, float* probs, int32_t* argmax, uint8_t* silent,
                           uint32_t flags);

/*
 * Speaker registration in a room, step 2 of the reference's manual: every speaker's recording (a
 * one-minute paragraph: SpeakerIdentification/scripts/record_on_pc.py:44-71,300-346) conditioned, cut
 * into 256-frame windows and embedded (make_feature_experiment and the frozen base of transfer_learning,
 * speaker_identification.py:317-369,401-432) on the context the room ticks on, in one call.
 *
 * mmla_si_enrol_embed: the conditioning is mmla_condition's with items_per_stream = 1 -- the gate passes
 *   against profile[c] of the context's bank (or MMLA_NR_NONSTATIONARY), the PCM_16 round trip per pass,
 *   lens, zeros behind kept_len -- with two differences.  clip_len may reach MMLA_ENROL_MAX_SAMPLES (the
 *   gate works chunk by chunk, as mmla_nr_reduce does for a long signal).  Silence removal runs on fresh,
 *   temporary detectors of mode vad_mode, one per recording: the context's mmla_vad_reset detectors, the
 *   capture converters and the noise bank are not touched.  (A stated deviation: the reference has one
 *   module-level Vad(3) for everything; a detector per recording is the room's detector per microphone.)
 *   Then mmla_si_features_seq_batch on the conditioned int16 with lens = kept_len, on the device, and
 *   SI-NET up to the BiLSTM output (mmla_si_embed's path, range guard and re-run policy) on all
 *   n_rec * w_max windows, w_max = ceil(T(clip_len) / 256).
 *   emb [n_rec, w_max, 512] f32: rows at or past n_windows[i] are the network's output on zero features
 *   and carry no meaning.  out_pcm [n_rec, clip_len] i16, kept_len [n_rec], n_windows [n_rec]: nullable.
 *   The result does not depend on mmla_set_microbatch (SI's size counts recordings per conditioning and
 *   windows per network pass; recordings are independent and the detectors fresh, so a repeated
 *   micro-batch starts again).  MMLA_E_INVALID: what mmla_condition rejects except its 600000 limit,
 *   clip_len > MMLA_ENROL_MAX_SAMPLES, vad_mode outside 0..3, a null emb; MMLA_E_NOWEIGHTS without SI
 *   weights; every check comes before any state moves.  With MMLA_DEVICE_PTR the call synchronises the
 *   context stream internally (its last launches are still only enqueued).
 * mmla_si_set_head: replaces the Dense head of the loaded SI model in place (the customized_dense of
 *   speaker_identification.py:407-432, or any Dense(K)): w [512, K], b [K], host pointers as for
 *   mmla_load_weights; head = MMLA_HEAD_SOFTMAX or MMLA_HEAD_SIGMOID.  Waits for the context stream,
 *   prepares the head exactly as mmla_load_weights does (the 3xFP16 split at the tensor's own scale; a
 *   non-finite tensor makes the whole model run exact f32, a finite one afterwards lifts that again
 *   unless the base itself is non-finite) and frees the old one: every later call gives the bits
 *   mmla_load_weights of the full blob with that head would give, without re-uploading the base.
 *   MMLA_E_NOWEIGHTS without an SI model; MMLA_E_INVALID: n_classes < 1, an unknown head, null pointers.
 */
#define MMLA_ENROL_MAX_SAMPLES 1966080 /* 4096 detector frames of 480 samples: the VAD's item limit */
int mmla_si_enrol_embed(mmla_ctx* ctx, const int16_t* pcm, int64_t n_rec, int64_t stride,
                        const int32_t* lens, int32_t clip_len, const int32_t* profile, int32_t nr_passes,
                        int32_t silence_remove, int32_t vad_mode, int16_t* out_pcm, int32_t* kept_len,
                        int32_t* n_windows, float* emb, uint32_t flags);
int mmla_si_set_head(mmla_ctx* ctx, const float* w, const float* b, int32_t n_classes, int32_t head);

/*
 * Rate conversion of the offline pre-conditioning (resample.hip).
 * mmla_ratecv: pydub AudioSegment.set_frame_rate(outrate) on 16-bit PCM, i.e.
 *   audioop.ratecv(data, 2, nch, inrate, outrate, None) (OverlapDetection/scripts/
 *   overlap_detection_post_processing.py:120-121; SpeakerIdentification/scripts/
 *   speaker_identification_post_processing.py:159-160), bit-identical to CPython's audioop.
 *   pcm [n_frames][nch] interleaved -> out [out_frames][nch]; out_frames must be
 *   (n_frames - 1) * (outrate / g) / (inrate / g) + 1 with g = gcd(inrate, outrate) (0 for no input).
 * mmla_resample_sinc: resampy.resample(x, sr_orig, sr_new, filter=<half window>) on one float32
 *   channel -- librosa.load(path) at its default 22050 Hz uses filter 'kaiser_best'
 *   (speaker_identification_post_processing.py:142).  half_window [window_len] float64 is the
 *   filter's right half sampled num_table times per zero crossing (resampy sinc_window); n_out must
 *   be int(n * sr_new / sr_orig).  resampy's float64 time register, filter interpolation and float32
 *   accumulation are reproduced (library absent here: parity against resampy itself unpinned).
 */
int mmla_ratecv(mmla_ctx* ctx, const int16_t* pcm, int64_t n_frames, int32_t nch, int32_t inrate,
                int32_t outrate, int16_t* out, int64_t out_frames, uint32_t flags);
int mmla_resample_sinc(mmla_ctx* ctx, const float* x, int64_t n, int32_t sr_orig, int32_t sr_new,
                       const double* half_window, int64_t window_len, int32_t num_table, float* y,
                       int64_t n_out, uint32_t flags);

/*
 * A room that ticks at its microphones' capture rate: streaming conversion of interleaved 16-bit capture
 * (USB microphones and conference arrays: 44.1 / 48 kHz, usually stereo) to the 16 kHz mono every other
 * call takes, with audioop's ratecv state carried per stream from clip to clip.  Replaces, per clip and
 * microphone on the host: np.fromstring(data, np.int16)[0::2] (SpeakerIdentification/scripts/
 * record_on_pi.py:223), pydub's set_channels(1) = audioop.tomono(data, 2, 0.5, 0.5) and set_frame_rate(16000)
 * = audioop.ratecv (overlap_detection_post_processing.py:120-121).  Bit-identical to CPython's audioop.
 *
 * The format: rate 1..384000 Hz, channels 1..8, channel = k >= 0 picks channel k of every frame,
 * MMLA_CAPTURE_MEAN (two channels only) is floor(0.5 l + 0.5 r).  The mono signal is formed first and
 * goes through audioop.ratecv(fragment, 2, 1, rate, 16000, state).  With ir = rate / g, or = 16000 / g,
 * g = gcd(rate, 16000), a stream's state is (d, prev): audioop's phase counter, -max(ir, or) <= d < 0
 * (fresh: -or), and the last mono input sample (fresh: 0).  A fragment of n frames x entered with
 * (d0, prev) gives m = floor((n or + d0) / ir) + 1 samples (0 when n or + d0 < 0); sample j comes from
 * frame k = ceil((j ir - d0) / or) - 1 at phase d = d0 + (k + 1) or - j ir:
 *   out[j] = ((int)(((double)p * d + (double)c * (or - d)) / (double)or)) >> 16,
 *   p = (k > 0 ? x[k - 1] : prev) * 65536, c = x[k] * 65536 (no fp contraction; the cast truncates, the
 *   shift floors), and leaves (d0 + n or - m ir, n > 0 ? x[n - 1] : prev).  n = 0 changes nothing.
 *
 * mmla_capture_reset: sets the context's format and gives each of n_streams streams a fresh state (waits
 *   for the context stream).  MMLA_E_INVALID: a rate, channel count or channel out of range,
 *   MMLA_CAPTURE_MEAN with channels != 2.
 * mmla_capture_convert: the conversion alone.  Clip c = pcm + c * clip_stride (int16 samples) holds
 *   frames[c] frames (nullable: clip_frames) of `channels` samples; stream s owns clips
 *   [s * items_per_stream, (s + 1) * items_per_stream), in order.  out [n_clips][out_stride] int16 gets
 *   out_lens[c] samples per clip, then zeros up to out_clip_len = (clip_frames * or - 1) / ir + 1, the
 *   longest a clip can become (out_stride >= out_clip_len).  Every stream's state advances once.
 *   With MMLA_CAPTURE_FRESH the conversion starts from fresh states instead and leaves the context's
 *   alone, for any stream count: a whole recording (ambient noise, registration) cut into the clips of
 *   one stream.  Host-pointer calls stage the raw capture on the device in pieces of whole streams
 *   (64 MiB, or one stream), not all at once.
 * mmla_capture_state: d [n_streams] and prev [n_streams] (host, each nullable) of the current states
 *   (waits for the context stream): for tests and for checkpointing a room.
 * mmla_{od,si,room}_pipeline_capture: the arguments of the _conditioned calls with frames / clip_frames
 *   in capture frames in place of lens / clip_len: the conversion of all clips, once, then the
 *   conditioned pipeline on the converted clips with lens = out_lens and clip_len = out_clip_len (so
 *   out_pcm is [n_clips, out_clip_len] and kept_len counts 16 kHz samples).  The converted audio stays
 *   on the device.  The conversion runs in front of the micro-batching: every converter state advances
 *   exactly once per clip whatever the micro-batch size, and a range-guard, split-BiLSTM or
 *   allocation-failure re-run re-reads the clips already converted.  MMLA_NR_NONSTATIONARY and
 *   MMLA_DEVICE_PTR mean what they mean for the _conditioned calls (frames is then a device pointer).
 * MMLA_E_INVALID (conversion and pipelines; every check, the weights' and the bank's included, comes
 *   before any state moves, and a call that fails a check leaves every state as it was): no
 *   mmla_capture_reset for n_clips / items_per_stream streams, n_clips not a multiple of
 *   items_per_stream, clip_frames < 1, clip_stride < clip_frames * channels, a host frames[c] outside
 *   [0, clip_frames] (device pointers: clamped by the kernels, the convention of the VAD's lens),
 *   out_clip_len > 600000, and for the pipelines everything mmla_condition rejects.
 */
#define MMLA_CAPTURE_MEAN (-1)
#define MMLA_CAPTURE_FRESH 0x4u /* mmla_capture_convert: from fresh states, the context's untouched */
int mmla_capture_reset(mmla_ctx* ctx, int64_t n_streams, int32_t rate, int32_t channels, int32_t channel);
int mmla_capture_convert(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                         const int32_t* frames, int32_t clip_frames, int64_t items_per_stream, int16_t* out,
                         int64_t out_stride, int32_t* out_lens, uint32_t flags);
int mmla_capture_state(mmla_ctx* ctx, int32_t* d, int32_t* prev);
int mmla_od_pipeline_capture(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                             const int32_t* frames, int32_t clip_frames, const int32_t* profile,
                             int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                             int16_t* out_pcm, int32_t* kept_len, float* probs, int32_t* argmax,
                             uint8_t* silent, uint32_t flags);
int mmla_si_pipeline_capture(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                             const int32_t* frames, int32_t clip_frames, const int32_t* profile,
                             int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                             int16_t* out_pcm, int32_t* kept_len, float* probs, int32_t* argmax,
                             uint8_t* silent, uint32_t flags);
int mmla_room_pipeline_capture(mmla_ctx* ctx, const int16_t* pcm, int64_t n_clips, int64_t clip_stride,
                               const int32_t* frames, int32_t clip_frames, const int32_t* profile,
                               int32_t nr_passes, int32_t silence_remove, int64_t items_per_stream,
                               int16_t* out_pcm, int32_t* kept_len, float* od_probs, int32_t* od_argmax,
                               float* si_probs, int32_t* si_argmax, uint8_t* silent, uint32_t flags);

/*
 * Kernel tracing (replaces the reference's time.time() prints, overlap_detector_run.py:49-104).
 * When enabled, every kernel launch is bracketed by hipEvents on the context stream and its device
 * time is accumulated per stage together with the stage's algorithmic work (bytes for the
 * front-ends, FLOPs for the networks).  mmla_profile_read waits for the recorded events.
 */
#define MMLA_NSTAGES 7
enum mmla_stage {
  MMLA_STAGE_OD_FE = 0, /* work = algorithmic HBM bytes; also the SSIM launches (2 images in + 4 B out) */
  MMLA_STAGE_SI_FE = 1, /* work = algorithmic HBM bytes */
  MMLA_STAGE_CONV = 2,  /* work = FLOPs (2 * MACs, unpadded) */
  MMLA_STAGE_LSTM = 3,  /* work = FLOPs */
  MMLA_STAGE_GLUE = 4,  /* stem, pooling, mean: work = FLOPs; VAD, PCM conversions: bytes */
  MMLA_STAGE_HEAD = 5,  /* dense + softmax / sigmoid, mmla_si_head_fit: work = FLOPs */
  MMLA_STAGE_NR = 6     /* noise gate: work = algorithmic HBM bytes (signal in + out) */
};
int mmla_profile_enable(mmla_ctx* ctx, int on);

/* Layer-wise parity tap (tests): run OD-NET on host float NHWC x[n,128,151,C] (the model's C) up to `stage`
 * (0 = stem conv, 1..9 = after res_block 1..9 in NHWC, 10 = mean over H [n,19,128],
 * 11 = BiLSTM output [n,512]) and copy that tensor to host `out` (capacity out_floats).
 * Unguarded: it shows what the selected arithmetic computes.  Env MMLA_DEBUG_TRACE_GUARD=1 at
 * mmla_create makes it a host-pointer micro-batch under the range guard (mmla_set_precision): an
 * operand out of range in a kernel up to `stage` re-runs the trace in exact f32 and counts in
 * mmla_range_check. */
int mmla_debug_od_trace(mmla_ctx* ctx, const float* x, int64_t n, int stage, float* out,
                        int64_t out_floats);
/* Its twin for SI-NET on host features x[n,256,39]: stage 0 = stem conv [n,256,32], 1..9 = after
 * res unit 1..9 ([n,128,32] x 3, [n,64,64] x 3, [n,32,128] x 3), 10 = final BN + ReLU + AvgPool4
 * [n,8,128], 11 = BiLSTM output [n,512] (mmla_si_embed's), 12 = the logits [n,K] (the first K columns
 * of each padded row).  The launches are the ones the context's switches select, whatever the stage:
 * a stage that such a launch keeps on chip (a unit inside a fused chain or pair; unit 9 under the
 * fused final epilogue, MMLA_NO_SIFIN unset) is MMLA_E_INVALID and mmla_last_error names the launch.
 * MMLA_DEBUG_TRACE_GUARD=1 as above; the launches behind `stage` do not run. */
int mmla_debug_si_trace(mmla_ctx* ctx, const float* x, int64_t n, int stage, float* out,
                        int64_t out_floats);
/* Debug (tests, tools): device address and size of internal workspace slot `slot` (0 and 0 when the
 * slot was never allocated), e.g. to check that no kernel of another call writes into it. */
int mmla_debug_ws_slot(mmla_ctx* ctx, int slot, void** ptr, size_t* bytes);
/* Debug (tests): recovery counters of the context so far (each nullable): host-pointer micro-batches
 * re-run in exact f32 by the range guard, and host-pointer micro-batches re-run on the
 * one-workgroup-per-direction BiLSTM because a workgroup of the split BiLSTM (batches <= 128 clips)
 * timed out waiting for the others.  Env MMLA_DEBUG_LSTM_SPIN=<polls> at mmla_create bounds that
 * wait (tests force the timeout path with 1). */
int mmla_debug_counters(mmla_ctx* ctx, int64_t* f32_reruns, int64_t* lstm_split_reruns);
/* Debug (tests, tools): *wave = 1 when a detector call of this context over n_streams streams runs the
 * one-stream-per-wave kernel, 0 for the one-thread-per-stream kernel (the same decisions and states bit
 * for bit).  Env at mmla_create: MMLA_NO_VADW=1 per thread everywhere, MMLA_VADW=1 per wave everywhere. */
int mmla_debug_vad_path(mmla_ctx* ctx, int64_t n_streams, int32_t* wave);
/* Debug (tests): the stationary gate's noise thresholds as the device holds them, copied to host
 * `thresh` as [n_profiles][513] f32 (dB) after a synchronisation of the context's stream; *n_profiles
 * (nullable) is the bank's size.  MMLA_E_INVALID without a bank (mmla_nr_set_noise / _bank) or when
 * cap_floats < n_profiles * 513. */
int mmla_debug_nr_thresh(mmla_ctx* ctx, float* thresh, int64_t cap_floats, int64_t* n_profiles);
/* ms[MMLA_NSTAGES], launches[MMLA_NSTAGES], work[MMLA_NSTAGES] (each nullable); reset != 0 clears */
int mmla_profile_read(mmla_ctx* ctx, double* ms, int64_t* launches, double* work, int reset);

#ifdef __cplusplus
}
#endif

#endif /* MMLA_H_ */
