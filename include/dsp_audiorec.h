/*
 * dsp_audiorec.h -- C ABI of the MI355X (gfx950) feature-extraction + KNN path.
 *
 * Drop-in boundary for the reference's hot path (Hypersonic-cpu/DSP-AudioRecLabs):
 * every entry point names the reference function(s) it replaces.  The reference is
 * pure Python, so its "FFI" is the Python module surface src/audio_processing.py,
 * src/feature_extraction.py and src/models.py; the host mirror of that surface
 * (dsp-audioreclabs_amd/src/) binds this header with ctypes.
 *
 * Conventions
 *  - All pointers are DEVICE pointers unless stated; buffers are caller-allocated.
 *  - Every launch is stream-ordered on `stream` (a hipStream_t passed as void*;
 *    NULL = the legacy default stream).  No entry point allocates, frees, copies
 *    to the host or synchronises, so all of them may be captured in a hipGraph.
 *  - Scratch buffers (workspace, queue_ws) belong to one launch at a time, like any
 *    scratch: launches that may run concurrently (other streams, other instances of a
 *    captured graph) need their own.  No entry point keeps state between launches.
 *  - Return value: 0 on success, a DSP_ERR_* code (argument checks, done on the
 *    host before launching), or DSP_ERR_HIP + hipError_t when a launch fails.
 *  - Per-item failures (the reference raises ValueError and its callers skip the
 *    file, experiments/run_experiments.py:109-111) are reported in `status[b]`.
 */
#ifndef DSP_AUDIOREC_H
#define DSP_AUDIOREC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSP_ABI_VERSION 6  /* 2: dsp_extract_features takes the clip-queue scratch (queue_ws);
                              3: queue_ws is 64 bytes (per-XCD chunk counters);
                              4: the batch WAV reader (dsp_wav_scan / dsp_wav_read);
                              5: queue_ws is 4 KiB (each counter on its own 256-B line);
                              6: the extraction entry points take out_stride (packed result rows);
                                 dsp_knn_classify takes flags (DSP_KNN_REF_READY).
                              Still 6 with the dsp_mlp_*, dsp_svc_*, dsp_gnb_*, dsp_tree_* and dsp_dtw_* (dsp_dtw_align, dsp_dtw_dba_update included) and dsp_hmm_* and dsp_vq_* and dsp_dhmm_* (dsp_dhmm_decode, dsp_dhmm_decode_grammar, dsp_dhmm_forward, dsp_dhmm_expect and dsp_dhmm_force_* included) and dsp_pitch_* and dsp_lpc_* entry points: new symbols only, no
                              existing signature or meaning changed, so callers built against 6 keep
                              working (a binding that needs them checks for the symbols) */

/* return codes */
#define DSP_OK 0
#define DSP_ERR_ARGS 1        /* bad sizes / null pointers / misaligned buffers */
#define DSP_ERR_TOO_LONG 2    /* a clip does not fit the on-chip (LDS) pipeline */
#define DSP_ERR_WORKSPACE 3   /* workspace too small */
#define DSP_ERR_HIP 1000      /* + hipError_t of the failed launch */

#define DSP_QUEUE_WS_BYTES 4096  /* dsp_extract_features' queue_ws */
#define DSP_OUT_ROW_WORDS 19     /* one clip's results as a packed row of 4-byte words: feat[15] (f32),
                                    start, end, n_frames, status (int32) -- 76 B */

/* per-clip status[b] (low byte) -- same codes as the oracle */
#define DSP_CLIP_OK 0
#define DSP_CLIP_EMPTY 1      /* zero-length clip: np.max of an empty array raises (audio_processing.py:72) */
#define DSP_CLIP_NO_AUDIO 2   /* "No audio remaining ..." (audio_processing.py:388-389) */
#define DSP_CLIP_NO_FRAMES 3  /* "No frames provided ..." (feature_extraction.py:27-28) */
#define DSP_CLIP_TOO_LONG 4   /* longer than the max_len given at launch (dsp_extract_general
                                 processes such clips) */
#define DSP_CLIP_UNCERTIFIED 5 /* internal, never left in status on return of the stream:
                                  the fused kernel marks a clip whose endpoint decision is a
                                  near tie (within the 1e-11 certification margin) with it, and
                                  the exact kernel that dsp_extract_features launches next on
                                  the same stream redoes every such clip on the bit-exact path */
/* status[b] flag bits (informational) */
#define DSP_CLIP_FLAG_VAD_EXACT 0x100 /* endpoint decision was a near tie: re-decided on the
                                         bit-exact (numpy-order) fp64 path */

/* Bytes of dynamic LDS dsp_extract_features needs for clips of up to max_len samples
 * (0 if it exceeds the 160 KiB of one CU). Host-only helper. */
size_t dsp_extract_lds_bytes(int64_t max_len, int frame_length, int frame_shift);
/* Diagnostic (host only): 1 when a dsp_extract_features launch with these arguments runs the
 * kernel with the compile-time LDS layout (the clip in registers; csrc/extract_layout.h
 * extract_fast_fits), 0 when it runs the runtime carve -- and 0 wherever dsp_extract_lds_bytes
 * returns 0.  Both layouts compute the same results; tests use it to know which one they reached. */
int dsp_extract_fast_layout(int64_t max_len, int frame_length, int frame_shift);

/*
 * dsp_extract_features -- fused per-clip pipeline: persistent workgroups (three per CU on the
 * compile-time layout), each taking one clip at a time -- its first clip by its own index, the
 * rest from a clip queue -- with the clip held in registers until its endpoints are decided and
 * the crop's frames re-read from L2.  A second launch on the same stream redoes near-tie endpoint
 * decisions on the bit-exact path (it returns at once when the first counted none in queue_ws).
 * Replaces, per clip, the chain
 *   preprocess            src/audio_processing.py:78-90   (remove_dc :49-59, normalize_audio :62-75)
 *   endpoint_detection    src/audio_processing.py:135-275 (when do_vad != 0)
 *   crop                  src/audio_processing.py:378
 *   frame_signal          src/audio_processing.py:299-333 (with create_window :278-296 supplied as `window`)
 *   extract_frame_features src/feature_extraction.py:12-43
 *   extract_statistical_features src/feature_extraction.py:65-88  (15-d vector)
 * as called per file by experiments/run_experiments.py:90-104.
 *
 * pcm       int16 samples of all clips back to back; clip b = pcm[offsets[b] .. offsets[b+1]).
 *           16-bit PCM as read by load_wav (:35-38); 8-bit PCM is passed as ((u8 - 128) mod 256),
 *           which is what load_wav's uint8 arithmetic computes (:31-34) -- any power-of-two
 *           scale cancels in preprocess.  `pcm` must be 16-byte aligned.
 * offsets   int64 [B+1], non-decreasing.
 * window    float64 [frame_length] = create_window(window_type, frame_length) (np.hamming etc.),
 *           zero only at its ends (true for the three reference windows).
 * hi/lo/zr  energy_high_ratio, energy_low_ratio, zcr_threshold_ratio (config.py:43-45).
 * max_len   longest clip in the batch (sizes the LDS carve-up; see dsp_extract_lds_bytes).
 * feat      float32 [B,15]: energy, magnitude, zcr x (mean, std, max, min, median).
 * start_end int32 [B,2]: start_point / end_point (0, len when do_vad == 0).
 * n_frames  int32 [B]: metadata['n_frames'] (frames after the crop).
 * status    int32 [B]: DSP_CLIP_* | flags.
 * out_stride 0: the four arrays above, each row-major as given.  >= DSP_OUT_ROW_WORDS: row b of
 *           each output starts b * out_stride 4-byte words after its pointer -- one packed row
 *           buffer rows[B][19] is feat = rows, start_end = rows + 15, n_frames = rows + 17, status
 *           = rows + 18, out_stride = 19: each clip's 76-B record is contiguous, so the per-clip
 *           results of a shard travel in one collective without packing.
 * vad_energy/vad_zcr (optional, may be NULL): float64 / int32 [B, ld_vad]: metadata energy_list,
 *           zcr_list (first (len-L)//S+1 entries; rows of clips with len < L are untouched).
 * seq       (optional, may be NULL): float32 [B, ld_seq, 3] per-frame (E, M, ZCR) -- the
 *           'sequence' method of extract_features_from_frames (:114-129); frames beyond
 *           ld_seq are dropped.
 * queue_ws  (optional, may be NULL): DSP_QUEUE_WS_BYTES (4096) bytes of device scratch, zero
 *           before the launch: the counters of the dynamic clip queue (persistent workgroups
 *           claim chunks of consecutive clips, from their own XCD's share first, so fast
 *           workgroups take more clips); the launch leaves it zero again, so it can be reused by
 *           the next launch on the same stream.  NULL: a static round-robin split of the clips
 *           over the workgroups (same results, slower).
 *           One launch at a time per queue_ws (see Conventions).
 */
int dsp_extract_features(const int16_t *pcm, const int64_t *offsets, int B, int64_t max_len,
                         int frame_length, int frame_shift, const double *window, int do_vad,
                         double hi, double lo, double zr, float *feat, int32_t *start_end,
                         int32_t *n_frames, int32_t *status, int out_stride, double *vad_energy,
                         int32_t *vad_zcr, int ld_vad, float *seq, int ld_seq, void *queue_ws,
                         void *stream);

/*
 * dsp_extract_general -- the same pipeline for clips outside the fused kernel's on-chip plan:
 * any length (process_audio_file has no limit, src/audio_processing.py:336-396) and samples
 * wider than int16: 16-bit stereo, whose exact sample is the sum of the two channels (load_wav
 * averages them, :35-44; the power-of-two scale cancels in preprocess).  One workgroup per clip
 * from global memory; results identical to dsp_extract_features' where both apply.
 *
 * pcm          int16 (sample_bytes 2) or int32 (sample_bytes 4) samples, clips at offsets[b].
 * clip_index   int32 [nclip] clip numbers b to process (device; NULL: b = 0 .. nclip-1).  Only
 *              clips with min_len < len <= max_len are processed (min_len = 0: every clip,
 *              empty ones reported DSP_CLIP_EMPTY and ones longer than max_len
 *              DSP_CLIP_TOO_LONG); with min_len > 0 the outputs of the others are untouched, so
 *              a batch can be split between the two entry points without a host round trip.
 * outputs      as dsp_extract_features, indexed by clip number b.
 * workspace    device scratch of dsp_extract_general_workspace_bytes(nclip, max_len, L, S).
 */
size_t dsp_extract_general_workspace_bytes(int64_t nclip, int64_t max_len, int frame_length,
                                           int frame_shift);
int dsp_extract_general(const void *pcm, int sample_bytes, const int64_t *offsets,
                        const int32_t *clip_index, int nclip, int64_t min_len, int64_t max_len,
                        int frame_length, int frame_shift, const double *window, int do_vad,
                        double hi, double lo, double zr, float *feat, int32_t *start_end,
                        int32_t *n_frames, int32_t *status, int out_stride, double *vad_energy,
                        int32_t *vad_zcr, int ld_vad, float *seq, int ld_seq, void *workspace,
                        size_t workspace_bytes, void *stream);

/*
 * KNN -- KNeighborsClassifier(n_neighbors=k) as configured in src/models.py:33-35 and used by
 * TraditionalClassifier.fit/predict (:52-58): exact Euclidean k nearest neighbours of each query
 * row among the reference rows, ascending distance, then a uniform majority vote in which the
 * smallest label wins ties (scipy.stats.mode).  Screening runs in fp32: for D < 16 / D < 32
 * (the 15-d features) in the expanded form |q|^2 + q'.r' on the matrix cores
 * (v_mfma_f32_16x16x4_f32, f32 in / f32 accumulate -- a deliberate departure from north_star's
 * "no MFMA", measured 6.9 -> 5.7 ms at 100k x 100k), for D = 16 / 32 in the
 * direct form (q - r)^2 on the VALU, for D > 32 in the direct form in chunks of 16.  The screen
 * only nominates candidates: its error bound (knn.hip knn_err_coeffs) holds for any summation
 * order inside an MFMA with at most one rounding per product and per addition, so the
 * certification below does not rest on the matrix core matching an fmaf chain bit for bit.
 * Survivors are re-ranked with the reference's own fp64 distance (sequential sum of squared
 * differences, no FMA, sqrt), and any query whose fp32 screen cannot certify the fp64 top-k is
 * re-solved exhaustively in fp64 on the device.  Exact-distance ties are ordered by smaller
 * reference index.
 *
 * Inputs must be finite: NaN or infinite components are outside the contract (scikit-learn
 * refuses them) and are not looked for.  Any finite magnitude whose fp64 squared distances are
 * finite is inside it: a query whose fp32 screen could have overflowed (|q|^2 + max |r|^2 not
 * below 2^125, knn.hip next to knn_err_coeffs) is not certified and goes to the exhaustive fp64
 * scan, and one whose screen underflowed fails the ordinary certification and goes there too.
 *
 * ref        float64 [Nr, D] row-major,  ref_labels int32 [Nr] in [0, n_classes)
 * query      float64 [Nq, D] row-major
 * self_offset  >= 0: query q is reference row self_offset + q and is excluded from its own
 *              neighbour list (kneighbors(X=None) semantics); -1: no exclusion.
 * idx        int32 [Nq, k] (-1 where fewer than k candidates), dist float64 [Nq, k] (+inf there),
 * pred       int32 [Nq] (may be NULL, or ref_labels NULL, to skip the vote: pred is then left
 *            untouched).  The vote is over the candidates there are; a query with no candidate
 *            at all (Nr = 0, or Nr = 1 and that row is the query's own) has no label: pred = -1.
 * workspace  device scratch of dsp_knn_workspace_bytes(Nr, Nq, D, k) bytes.  Its first part holds
 *            the reference set converted for the screen, at offsets that depend on (Nr, D) only.
 * flags      DSP_KNN_REF_READY: the workspace already holds that conversion, left by an earlier call
 *            with the same ref, Nr, D and k on the same stream (any Nq): the conversion -- the
 *            fit() side of KNeighborsClassifier, src/models.py:52-55 -- is skipped.  0: convert.
 * Requires 1 <= D <= 4096, 1 <= k <= 32.  D <= 32: queries in registers, reference tiles in LDS;
 * D > 32 (the sequence method's flattened features): dimensions walked in chunks of 16.
 */
#define DSP_KNN_REF_READY 1
size_t dsp_knn_workspace_bytes(int64_t Nr, int64_t Nq, int D, int k);
/* Diagnostic: byte offset in that workspace of an int32 that dsp_knn_classify leaves holding the
 * number of queries the screen could not certify (answered by the exhaustive fp64 fallback). */
size_t dsp_knn_workspace_fallbacks_offset(int64_t Nr, int64_t Nq, int D, int k);
int dsp_knn_classify(const double *ref, const int32_t *ref_labels, int64_t Nr, const double *query,
                     int64_t Nq, int D, int k, int64_t self_offset, int n_classes, int32_t *idx,
                     double *dist, int32_t *pred, void *workspace, size_t workspace_bytes, int flags,
                     void *stream);

/*
 * normalize_features (src/feature_extraction.py:157-181): column mean and population std
 * (ddof = 0), std == 0 -> 1, then (X - mean) / std, bit for bit np.mean / np.std over axis 0 of
 * a C-contiguous [N, D] array.  That is numpy's summation order, which depends on D:
 *   D >= 2  each column sequentially over the rows;
 *   D == 1  numpy coalesces the axes and sums the one contiguous column in chunks of 8192 rows
 *           (its buffer), adding the chunks' sums in order, and each chunk of n rows pairwise: in
 *           order for n < 8; for n <= 128 eight running sums over strides of 8 combined as
 *           ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the n % 8 tail in order; otherwise split at
 *           n / 2 rounded down to a multiple of 8, recursively.  The std sums (x - mean)^2 alike.
 * dsp_zscore_fit writes mean/std [D] (std already with the 0 -> 1 substitution);
 * dsp_zscore_apply writes out [N, D] (may alias X).  float64 throughout, X row-major.
 */
int dsp_zscore_fit(const double *X, int64_t N, int D, double *mean, double *std, void *stream);
int dsp_zscore_apply(const double *X, int64_t N, int D, const double *mean, const double *std,
                     double *out, void *stream);

/*
 * MLP classifier -- MLPClassifier / MLPTrainer of src/models.py:77-221: Linear -> ReLU -> Dropout per
 * hidden layer, a last Linear, CrossEntropyLoss (mean over the actual batch), optim.Adam defaults
 * (betas 0.9 / 0.999, eps 1e-8, bias correction, no weight decay), strictly serial SGD over
 * shuffled batches.  float32 parameters, activations and accumulation; every sum in a fixed order
 * (no atomics), so equal inputs give equal bits.
 *
 * Packed parameter layout ("params", and the Adam moments m, v): layer after layer, PyTorch's
 * nn.Linear weight [out, in] row-major, then its bias [out] -- the tensors of the module's
 * state_dict() in order, flattened.  dsp_mlp_param_count gives the length P.
 *
 * Dropout hash (32-bit mixer "lowbias32", all arithmetic mod 2^32):
 *   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *   key  = mix(mix(mix(mix(seed + 0x9e3779b9) ^ low32(step)) ^ high32(step)) ^ layer)
 *   hash = mix(mix(key ^ row) ^ unit)
 * seed: the model's seed; step: optimizer steps the model has completed before this one (the
 * int64 step count, so it runs on across launches); layer: hidden layer index from 0; row: row
 * within the batch; unit: index within the layer.  A unit is dropped iff hash < drop_threshold
 * (drop_threshold = floor(p * 2^32); 0 = no dropout); kept units are multiplied by keep_scale,
 * the float32 value of 1 / (1 - p).  The hash depends on nothing else: not on launch boundaries,
 * not on n_models, not on the block a model runs in.
 */
#define DSP_MLP_MAX_HIDDEN 4
/* Host helpers.  dsp_mlp_lds_bytes: bytes of LDS dsp_mlp_train needs for batches of up to
 * batch_size rows, or 0 when the configuration is outside the fused plan (D, every hidden width and
 * C in 1..64, at most DSP_MLP_MAX_HIDDEN hidden layers, parameters + one batch of activations
 * within the 160 KiB of one CU).  dsp_mlp_param_count: P (0 for bad sizes). */
size_t dsp_mlp_lds_bytes(int D, int n_hidden, const int *hidden, int C, int batch_size);
int64_t dsp_mlp_param_count(int D, int n_hidden, const int *hidden, int C);
/*
 * dsp_mlp_train -- MLPTrainer.fit's loop (src/models.py:146-194) for n_models independent models,
 * one persistent workgroup each, n_epochs epochs in one launch with no host round trip (the
 * reference syncs once per step, loss.item() :181).
 *
 * X          float32 [N, D] (FloatTensor(X_train) :156), y int32 [N] in [0, C) (clamped into it).
 *            Model k reads X + k * x_stride and y + k * y_stride (in elements): 0 = all models share
 *            the set (a learning-rate sweep), else >= N * D / >= N: one set per model, all of N rows
 *            (the window comparison's three feature sets, run_experiments.py:343-376).
 * hidden     HOST int [n_hidden].
 * perm       int32 [n_epochs, N] per model: epoch e visits rows perm[e][0..N) in consecutive batches
 *            of batch_size, the last one short (DataLoader(shuffle=True), drop_last=False :161);
 *            values are clamped into [0, N).  Model k reads perm + k * perm_stride (in elements):
 *            0 = all models share one order, else >= n_epochs * N.
 * params, m, v  float32 [n_models, P], in/out.  steps int64 [n_models], in/out: optimizer steps done.
 *            A second launch continues exactly where the first stopped.
 * lr         float64 [n_models] (device).  seeds uint32 [n_models] (device).
 * loss_hist, acc_hist  float32 [n_models, n_epochs]: per epoch the mean of the batches' mean losses
 *            (:181,:187) and correct / total over the train-mode outputs, first-index argmax (:182-188).
 * Returns DSP_ERR_ARGS outside the fused plan (dsp_mlp_lds_bytes == 0).
 */
int dsp_mlp_train(const float *X, const int32_t *y, int64_t N, int64_t x_stride, int64_t y_stride, int D,
                  int n_hidden, const int *hidden, int C, int n_models, int n_epochs, int batch_size,
                  const int32_t *perm,
                  int64_t perm_stride, float *params, float *m, float *v, int64_t *steps,
                  const double *lr, const uint32_t *seeds, uint32_t drop_threshold, float keep_scale,
                  float *loss_hist, float *acc_hist, void *stream);
/*
 * dsp_mlp_predict -- MLPTrainer.predict (src/models.py:196-205): the eval-mode forward pass (no
 * dropout) of one model over X float32 [Nq, D]; pred int32 [Nq] = first-index argmax (torch.max
 * :203); logits float32 [Nq, C] or NULL.  64 rows per workgroup, the weights staged in LDS.
 */
int dsp_mlp_predict(const float *params, const float *X, int64_t Nq, int D, int n_hidden,
                    const int *hidden, int C, int32_t *pred, float *logits, void *stream);
/* Diagnostic: mask uint8 [rows, width] = 1 where the unit is kept, by the trainer's own device
 * function (nn.Dropout's mask, src/models.py:97). */
int dsp_mlp_dropout_mask(uint32_t seed, int64_t step, int layer, int rows, int width,
                         uint32_t drop_threshold, uint8_t *mask, void *stream);

/*
 * SVC prediction -- SVC(kernel='rbf').predict of a model fitted by scikit-learn (libsvm), as
 * configured in src/models.py:44-47 and used by TraditionalClassifier.predict / evaluate (:56-58).
 * Training stays libsvm's; the fitted model is passed as libsvm holds it (scikit-learn's underscore
 * attributes -- the public dual_coef_ / intercept_ are sign-flipped for two classes):
 *   sv         float64 [nSV, D]     support_vectors_, grouped by class
 *   n_support  int32   [C]          _n_support (rows of sv per class, summing to nSV)
 *   dual_coef  float64 [C-1, nSV]   _dual_coef_
 *   intercept  float64 [C(C-1)/2]   _intercept_ (= -rho), in libsvm's pair order p: (0,1), (0,2), ...
 *   gamma                            _gamma
 * For each row of query float64 [Nq, D]:
 *   K_s   = exp(-gamma * sum_d (q_d - sv[s][d])^2)            (the direct form, fp64)
 *   dec_p = sum_{s in class i} dual_coef[j-1][s] K_s + sum_{s in class j} dual_coef[i][s] K_s
 *           + intercept[p]                                     for the pair i < j
 *   a vote for i if dec_p > 0, else for j; pred = the first class index with the most votes
 *   (SVC.predict is classes_[pred]).
 * dec        float64 [Nq, C(C-1)/2] with libsvm's signs, or NULL.  For C > 2 this is
 *            decision_function with decision_function_shape='ovo'; for C == 2 its negation.
 * certified  int32 [Nq]: 1 when every |dec_p| exceeds four times the derived bound on
 *            |dec_device - dec_libsvm| (any summation order on both sides, a few ulp per exp, the
 *            rounding of the squared distance), so the vote is libsvm's; 0: the
 *            caller answers that row with libsvm itself.  Equal inputs give equal bits, and a row's
 *            dec bits do not depend on Nq or on the row's position (fixed summation order, no atomics
 *            on floating-point data).  A query row holding an inf or a NaN (scikit-learn refuses it)
 *            comes back with NaN in every dec_p and certified = 0, and is counted.
 * workspace  device scratch of dsp_svc_workspace_bytes(nSV, Nq, D, C) bytes (0: sizes outside the
 *            plan); at dsp_svc_workspace_uncertified_offset an int32 is left holding the number of
 *            uncertified rows.
 * dsp_svc_launch_parts (diagnostic, host only): 1 when a call of these sizes runs the query-tiled
 *            launch (a workgroup walks all support vectors), else the number of support-vector
 *            segments the launch is split over (few queries against many support vectors).
 * Requires 1 <= D <= 4096 (D <= 32: the query in registers, else dimensions in chunks of 16),
 * 2 <= C <= 64, 1 <= nSV < 2^31, gamma >= 0.
 */
size_t dsp_svc_workspace_bytes(int64_t nSV, int64_t Nq, int D, int C);
size_t dsp_svc_workspace_uncertified_offset(int64_t nSV, int64_t Nq, int D, int C);
int dsp_svc_launch_parts(int64_t nSV, int64_t Nq, int D, int C);
int dsp_svc_predict(const double *sv, const int32_t *n_support, const double *dual_coef,
                    const double *intercept, int64_t nSV, int D, int C, double gamma,
                    const double *query, int64_t Nq, int32_t *pred, double *dec, int32_t *certified,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Gaussian Naive Bayes -- GaussianNB().fit / .predict as configured in src/models.py:37-39 (no
 * priors, no sample weights) and used by TraditionalClassifier.fit / predict (:52-58).
 *
 * dsp_gnb_fit: X float64 [N, D] and y int32 [N], class codes in [0, C) (the index into classes_).
 *   theta        float64 [C, D]  theta_: the column sums over the class's rows, added in row order,
 *                                divided by the class's count
 *   var          float64 [C, D]  var_: sum (x - theta)^2 in row order, divided by the count, + epsilon
 *   class_count  int64   [C]     class_count_
 *   epsilon      float64 [1]     epsilon_ = var_smoothing * the largest all-rows column variance
 *                                (np.var(X, axis=0).max(), the same two passes over all rows)
 *   These are numpy's own sequential fp64 chains (axis 0, D >= 2), neither reordered nor atomic:
 *   the four arrays equal GaussianNB().fit's bit for bit.  A chain starts from +0.0, np.add.reduce's
 *   own start: a class whose rows are all -0.0 in a column has the mean +0.0 there, not -0.0.  class_prior_ is class_count /
 *   class_count.sum(), the caller's.
 *   workspace    device scratch of at least 8 D bytes.
 *   A class without rows gets class_count 0 and NaN in its theta and var rows (0 / 0); a row whose
 *   code is outside [0, C) counts for epsilon only.  A NaN or an inf in a column makes that column's
 *   var NaN, and -- as np.var(X, axis=0).max() does -- epsilon and with it every var NaN.
 *   Requires 2 <= D <= 4096 (D = 1: DSP_ERR_ARGS -- numpy sums that case pairwise), 1 <= C <= 64,
 *   N >= 1.
 *
 * dsp_gnb_predict: theta, var float64 [C, D] (var_ with epsilon, as fitted), log_prior float64 [C]
 * = np.log(class_prior_), nconst float64 [C] = -0.5 * np.sum(np.log(2 pi var_), axis=1) (the
 * caller computes both with numpy, as _joint_log_likelihood does).  For each row of X float64 [Nq, D]:
 *   Q_c   = sum_d (x_d - theta[c][d])^2 / var[c][d]       (fp64, added in column order)
 *   jll_c = log_prior[c] + (nconst[c] - 0.5 Q_c)
 *   pred  = the first index of the largest jll (GaussianNB.predict is classes_[pred])
 * jll        float64 [Nq, C], or NULL.
 * certified  int32 [Nq]: 1 when every score is finite and jll_pred - jll_c exceeds four times
 *            (bound_pred + bound_c) for every other class c,
 *              bound_c = 2 (D + 8) 2^-53 (|log_prior[c]| + |nconst[c]| + Q_c / 2)
 *            the derived bound on |jll_device - jll_sklearn|, so the label is
 *            scikit-learn's; 0: the caller answers that row with scikit-learn itself (a row with a
 *            NaN or an infinity is never certified).  Equal inputs give equal bits, and a row's bits
 *            do not depend on Nq or on the row's position.
 *            A score that is not finite -- Q_c overflows (a finite x whose (x - theta)^2 or quotient
 *            overflows included), log_prior[c] = -inf, a class with NaN parameters -- leaves the whole
 *            row uncertified, whichever class leads.  pred is taken with ">" from class 0 on: equal
 *            scores (duplicate classes) give the first index and no certificate, and a NaN score
 *            never replaces a leader (pred is then the caller's to redo, as for every uncertified row).
 *            C = 1 is certified whenever its score is finite.
 * workspace  device scratch of dsp_gnb_workspace_bytes(Nq, D, C) bytes (0: sizes outside the plan);
 *            its first int32 is left holding the number of uncertified rows (0 for Nq = 0).  The
 *            count is cleared by a kernel's store, so the call is a plain chain of kernels on
 *            `stream` and may be captured in a graph and replayed: every replay recounts.
 * Requires 1 <= D <= 4096 (D <= 32: the query in registers), 1 <= C <= 64.
 */
int dsp_gnb_fit(const double *X, const int32_t *y, int64_t N, int D, int C, double var_smoothing,
                double *theta, double *var, int64_t *class_count, double *epsilon, void *workspace,
                size_t workspace_bytes, void *stream);
size_t dsp_gnb_workspace_bytes(int64_t Nq, int D, int C);
int dsp_gnb_predict(const double *theta, const double *var, const double *log_prior, const double *nconst,
                    int D, int C, const double *X, int64_t Nq, int32_t *pred, double *jll,
                    int32_t *certified, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Decision tree prediction -- DecisionTreeClassifier.predict / .apply of a fitted single-output
 * tree (src/models.py:40-43, :56-58).  Training stays scikit-learn's.  The tree as tree_ holds it:
 *   children_left, children_right, feature  int32 [n_nodes]   (children_left == -1: a leaf)
 *   threshold                               float64 [n_nodes]
 *   leaf_class                              int32 [n_nodes]   np.argmax(tree_.value[:, 0, :], axis=1)
 *   max_depth                               tree_.max_depth
 * For each row of X float64 [Nq, D]: from node 0, v = (double)(float)x[feature] (to nearest even,
 * scikit-learn's float32 cast), left iff v <= threshold, until a leaf.
 *   pred  int32 [Nq]  leaf_class of the leaf (predict is classes_[pred])
 *   leaf  int32 [Nq]  the leaf's node index (apply), or NULL
 * A row that holds a NaN, or a value that is not finite as float32, gets pred = leaf = -1
 * (scikit-learn treats a NaN as a missing value and refuses the others: the caller hands the row to
 * it).  The walk ends on any
 * table: at most max_depth + 1 nodes are visited, and a child index outside (node, n_nodes) or a
 * feature index outside [0, D) ends it with pred = leaf = -1.
 * A threshold is compared as a double: one outside the float32 range or between two float32
 * subnormals decides as written (float32 subnormals are not flushed; x = -0.0 <= +0.0 and
 * +0.0 <= -0.0 go left).  A NaN threshold compares false with every value: the walk goes right.  A
 * double that rounds to +-inf as float32 -- the midpoint between FLT_MAX and 2^128 rounds to even,
 * which is inf -- is not finite as float32.
 * workspace  device scratch of dsp_tree_workspace_bytes(n_nodes) bytes (the packed 16-byte nodes);
 *            its first int32 is left holding the number of rows answered -1 (0 for Nq = 0).  The
 *            count is cleared by a kernel's store (as dsp_gnb_predict's): the call may be captured
 *            in a graph and replayed.
 * dsp_tree_lds_nodes (host only): up to this many nodes the walk reads the table from LDS, beyond
 *            it from memory.
 * Requires 1 <= n_nodes < 2^31, max_depth >= 0, 1 <= D <= 4096.
 */
size_t dsp_tree_workspace_bytes(int64_t n_nodes);
int dsp_tree_lds_nodes(void);
int dsp_tree_predict(const int32_t *children_left, const int32_t *children_right, const int32_t *feature,
                     const double *threshold, const int32_t *leaf_class, int64_t n_nodes, int max_depth,
                     int D, const double *X, int64_t Nq, int32_t *pred, int32_t *leaf, void *workspace,
                     size_t workspace_bytes, void *stream);

/*
 * Dynamic time warping (DTW) and its k nearest neighbours -- the textbook classifier for the
 * per-frame (E, M, ZCR) sequences that dsp_extract_features writes to `seq` (the reference only
 * zero-pads and flattens them, compare_feature_methods.py:106-115).  csrc/dtw.hip, DESIGN.md §4.8.
 *
 * Sequences are float64, padded row-major: a [Nq, Tq, F] with len_a int32 [Nq], b [Nr, Tr, F] with
 * len_b int32 [Nr]; 1 <= F <= 8, 1 <= Tq, Tr <= 1024.  For a pair with lengths n, m:
 *   c(i,j) = sum_f (a[i,f] - b[j,f])^2    f ascending, fp64, each product and each sum rounded (no FMA)
 *   D(0,0) = c(0,0)
 *   D(i,j) = c(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1))   neighbours outside the grid or the band are +inf
 *   dtw    = sqrt(D(n-1, m-1))
 * window < 0: unconstrained.  window >= 0: a Sakoe-Chiba band, cell (i,j) admissible iff
 * |i - j| <= max(window, |n - m|), so the end cell is always reachable.
 * Only fp64 subtract, multiply, add, min and sqrt occur, all correctly rounded, and min is
 * order-independent on non-negative finite values: the result is defined bit for bit, and a pair's
 * bits do not depend on Nq, Nr, the pair's position, the tile it lands in or the launch shape.
 * A sequence whose length is < 1 or greater than its padded width has distance +inf to everything;
 * no row is read outside its padded width.  Non-finite sample values: the result is unspecified (the
 * Python surface rejects them), but the kernel terminates and stays in bounds.
 *
 * dsp_dtw_pairwise: dist float64 [Nq, Nr].
 * dsp_dtw_knn: the k nearest reference sequences of each query under dtw, by dsp_knn_classify's
 *   rules: 1 <= k <= 32, ascending distance (the dtw value dsp_dtw_pairwise returns), exact-distance
 *   ties ordered by the smaller reference index, idx = -1 and dist = +inf where fewer than k
 *   references at a finite distance exist, self_offset >= 0 excludes reference row self_offset + q,
 *   a uniform vote in which the smallest label wins ties (pred = -1 without any neighbour); a NULL
 *   pred or NULL ref_labels skips the vote.  ref_labels int32 [Nr] >= 0; n_classes is informational.
 *   idx int32 [Nq, k], dist float64 [Nq, k], pred int32 [Nq].
 * workspace  device scratch of dsp_dtw_workspace_bytes(Nr, Nq, Tr, Tq, F, k) bytes (0: sizes outside
 *   the plan -- the limits above, 1 <= k <= 32, Nr < 2^31).  It stays bounded whatever Nq is: both
 *   entry points work through the queries in chunks of at most 1024 queries and at most 64 MiB of
 *   distance rows (one row when a single row is larger), and the workspace holds, for one chunk, the
 *   strips' edge columns of at most 4096 resident waves (at most 256 MiB, and only when Tq > 32), a
 *   copy of the chunk's queries behind 32 frames of zeros (at most 1024 x 1056 x F doubles, 66 MiB)
 *   and, for dsp_dtw_knn, the chunk's distance rows -- never the full [Nq, Nr] matrix.
 *   dsp_dtw_pairwise writes its rows straight to dist and accepts any workspace that holds the first
 *   two parts; the size for k = 1 always does.
 */
size_t dsp_dtw_workspace_bytes(int64_t Nr, int64_t Nq, int Tr, int Tq, int F, int k);
int dsp_dtw_pairwise(const double *a, const int32_t *len_a, int64_t Nq, int Tq, const double *b,
                     const int32_t *len_b, int64_t Nr, int Tr, int F, int window, double *dist,
                     void *workspace, size_t workspace_bytes, void *stream);
int dsp_dtw_knn(const double *ref, const int32_t *len_ref, const int32_t *ref_labels, int64_t Nr, int Tr,
                const double *query, const int32_t *len_query, int64_t Nq, int Tq, int F, int window,
                int k, int64_t self_offset, int n_classes, int32_t *idx, double *dist, int32_t *pred,
                void *workspace, size_t workspace_bytes, void *stream);

/*
 * DTW alignment paths and one DTW barycentre averaging (DBA; Petitjean, Ketterlin, Gancarski 2011)
 * update on them.  csrc/dtw_align.hip, DESIGN.md §4.9.  c, D, the band, the plan (1 <= F <= 8,
 * 1 <= T <= 1024) and invalid lengths are those above, unchanged.
 *
 * Path.  For a pair with lengths n (side a, index i) and m (side b, index j) the path is found by
 * walking back from (n-1, m-1) to (0, 0): the predecessor of (i, j) is the first of (i-1, j-1),
 * (i-1, j), (i, j-1) whose D equals the minimum of the three; neighbours outside the grid or the
 * band count as +inf.  D is defined bit for bit, so the path is.  dtw(a, b) and dtw(b, a) have equal
 * bits, but the tie rule is stated in a / b indices and is NOT symmetric.
 * Ranges.  The path is returned from a's side as two int32 rows per pair: frame i of a is matched to
 * frames lo[i] .. hi[i] of b.  lo[0] = 0, hi[n-1] = m-1 and hi[i] <= lo[i+1] <= hi[i] + 1; the
 * path's cells are exactly {(i, j): lo[i] <= j <= hi[i]}.  Entries i >= n are -1.  A pair with an
 * invalid length on either side gives dist = +inf and all entries -1.
 * Pairs are a CSR list over a: group_start int32 [Na + 1] (non-decreasing, group_start[0] = 0),
 * members int32 [P], P = group_start[Na] passed by the host (P < 2^31).  The sequences aligned to
 * a[c] are b[members[p]] for p in [group_start[c], group_start[c+1]); outputs are indexed by p.  A b
 * sequence may appear under several a's; a group may be empty.  A members entry outside [0, Nb) is
 * treated as an invalid length and never read through.
 *
 * dsp_dtw_align: dist float64 [P] (the dtw value of dsp_dtw_pairwise; may be NULL), lo and hi int32
 *   [P, Ta] (both or neither NULL; without them no path is walked).
 * dsp_dtw_dba_update: one DBA iteration for all templates in one call.  tmpl [C, Tt, F] with len_t,
 *   seqs [N, Ts, F] with len_s, the CSR list over the templates.  For template c of length L with
 *   valid-length members k0 < k1 < ... in list order:
 *     S_k[i,f] = s_k[lo,f] + s_k[lo+1,f] + ... + s_k[hi,f]     left to right, each sum rounded
 *     acc[i,f] = S_k0[i,f];  acc = acc + S_k for k1, k2, ...   in list order
 *     cnt[i]   = sum_k (hi - lo + 1)                           integer
 *     new[i,f] = acc[i,f] / (double)cnt[i]                     one rounded division
 *     inertia  = D_k0(end);  inertia = inertia + D_k(end)      dtw^2 (before the sqrt), in list order
 *   with lo, hi the ranges of the pair (template c, member k).  Rows i >= L of tmpl_out [C, Tt, F]
 *   are zeros.  tmpl_out[c] is a bitwise copy of tmpl[c] and its inertia 0.0 when the template's own
 *   length is invalid or it has no valid member; members with an invalid length are skipped.
 *   inertia float64 [C] may be NULL.  tmpl_out must not be tmpl.
 * workspace  device scratch of dsp_dtw_align_workspace_bytes(Na, P, Ta, Tb, F) bytes for both (C, Tt, Ts
 *   for Na, Ta, Tb; 0: sizes outside the plan).  It stays bounded whatever Na and P are: per
 *   resident wave (at most 4096, and at most 1 GiB of them) the predecessor codes of one tile --
 *   ceil(Ta / 32) x Tb x 64 words of 8 bytes -- and its edge column; the padded copy of one chunk of
 *   at most 1024 a sequences; and, for the DBA, the ranges and the sums S_k of one chunk of pairs
 *   (at most 128 MiB together) and the counts of one chunk of templates.
 * Both check their host arguments before any launch (DSP_ERR_ARGS, DSP_ERR_WORKSPACE), return DSP_OK
 * with nothing to do, make no host synchronisation and no allocation, and write only to their
 * outputs and the workspace, on the caller's stream.
 */
size_t dsp_dtw_align_workspace_bytes(int64_t Na, int64_t P, int Ta, int Tb, int F);
int dsp_dtw_align(const double *a, const int32_t *len_a, int64_t Na, int Ta, const double *b,
                  const int32_t *len_b, int64_t Nb, int Tb, int F, int window, const int32_t *group_start,
                  const int32_t *members, int64_t P, double *dist, int32_t *lo, int32_t *hi, void *workspace,
                  size_t workspace_bytes, void *stream);
int dsp_dtw_dba_update(const double *tmpl, const int32_t *len_t, int64_t C, int Tt, const double *seqs,
                       const int32_t *len_s, int64_t N, int Ts, int F, int window, const int32_t *group_start,
                       const int32_t *members, int64_t P, double *tmpl_out, double *inertia, void *workspace,
                       size_t workspace_bytes, void *stream);

/*
 * Left-to-right Gaussian hidden Markov models on the frame sequences, in the negative-log domain,
 * with the pieces of Viterbi training (segmental k-means).  csrc/hmm.hip, DESIGN.md §4.10.  Every
 * output is defined bit for bit: the device computes fp64 subtract, multiply, add, min and (in the
 * re-estimation) divide in the order below, each operation rounded, no FMA; the logarithms are the
 * caller's, taken when the model is built.
 *
 * Sequences: x float64 [N, T, F] padded row-major with len int32 [N], 1 <= F <= 8, 1 <= T <= 1024
 *   (the DTW plan above).
 * Model set: C <= 2^20 models padded to Smax states, 1 <= n_states[c] <= Smax <= 32: mu, w float64
 *   [C, Smax, F], g, stay, adv float64 [C, Smax], n_states int32 [C].  All finite or +inf, never NaN,
 *   never -inf (w = 0.5 / var, g = 0.5 sum_f log(2 pi var_f), stay = -log p_stay,
 *   adv = -log(1 - p_stay)); adv[c, S-1] is never read.
 * Recurrence, for a sequence of length n and a model of S states:
 *     e(t,s) = g[s];  for f ascending:  d = x[t,f] - mu[s,f];  e = e + w[s,f] * (d * d)
 *     V(0,0) = e(0,0);  V(0,s>0) = +inf
 *     a = V(t-1,s) + stay[s];  b = V(t-1,s-1) + adv[s-1]        (b = +inf at s = 0)
 *     V(t,s) = e(t,s) + min(a, b)
 *     score  = V(n-1, S-1)
 *   score is +inf when n < S, and also when n < 1, n > T or n_states[c] is outside 1 .. Smax.
 * Path: walk back from (n-1, S-1); the predecessor is the advance (t-1, s-1) iff b < a strictly, so
 *   ties stay.  Returned as seg int32 [P, Smax], seg[s] the first frame of state s: seg[0] = 0, seg is
 *   strictly increasing, entries s >= S are -1; every entry of a pair whose score is +inf is -1.
 * Pairs (dsp_hmm_align, dsp_hmm_accumulate): dsp_dtw_align's CSR list over the models -- group_start
 *   int32 [C + 1], members int32 [P]; a members entry outside [0, N) counts as an invalid length and
 *   is never read through; a sequence may appear under several models; a group may be empty.
 *
 * dsp_hmm_score: every sequence against every model, score float64 [N, C]; label int32 [N] the model
 *   index of the smallest score, ties to the smaller index, -1 when every score is +inf.  Either
 *   output may be NULL.
 * dsp_hmm_align: score float64 [P] and seg int32 [P, Smax] of the listed pairs; either may be NULL
 *   (without seg no direction bit is stored and no path is walked).
 * dsp_hmm_accumulate: the re-estimation of every model from a GIVEN seg [P, Smax] and score [P] (the
 *   output of dsp_hmm_align, or a segmentation of the caller's, e.g. the uniform start: state s =
 *   frames floor(s n / S) .. floor((s+1) n / S) - 1 for members with n >= S, -1 rows otherwise).  A
 *   member is valid when its index and length are and its seg row is well formed for its model
 *   (seg[0] = 0, strictly increasing over the S states, seg[S-1] < n); other members are skipped.
 *   For model c with valid members k0 < k1 < ... in list order, state s owning the member's frames
 *   beg = seg[s] .. end = seg[s+1] - 1 (the last state up to n - 1):
 *     X_k[s,f] = x[beg,f] + ... + x[end,f]        left to right; Q_k likewise over the products x * x
 *     accX = X_k0;  accX = accX + X_k  ...        in list order; accQ likewise
 *     cnt[s]   = sum_k (end - beg + 1)            integer
 *     mean = accX / cnt;   var = max(accQ / cnt - mean * mean, var_floor)
 *     total = score_k0 + score_k1 + ...           in list order;  n_valid = number of valid members
 *   Outputs mean, var float64 [C, Smax, F] (neither may be mu_prev / var_prev), cnt int32 [C, Smax],
 *   n_valid int32 [C], total float64 [C].  Rows s >= S are zeros.  A model with no valid member or
 *   an n_states outside 1 .. Smax is copied bit for bit from mu_prev / var_prev, with total 0.0,
 *   n_valid 0 and cnt 0.  Every valid member visits every state, so the transition estimate needs
 *   only these: p_stay[s] = (cnt[s] - n_valid) / cnt[s].
 * workspace  device scratch of dsp_hmm_workspace_bytes(C, N, P, T, F, Smax) bytes (0: sizes outside
 *   the plan; P = 0 for dsp_hmm_score): the model set repacked as one record per state, one 32-bit
 *   direction word per row and lane for each resident wave (at most 256 MiB), N x C scores (labels
 *   without scores), and for the re-estimation the sums of one chunk of pairs (at most 128 MiB) and
 *   the models' counts.  Nothing in it is carried from one call to the next.
 * All three check their host arguments before any launch (DSP_ERR_ARGS, DSP_ERR_WORKSPACE), return
 * DSP_OK with nothing to do, make no host synchronisation and no allocation, and write only to their
 * outputs and the workspace, on the caller's stream.
 */
size_t dsp_hmm_workspace_bytes(int64_t C, int64_t N, int64_t P, int T, int F, int Smax);
int dsp_hmm_score(const double *mu, const double *w, const double *g, const double *stay, const double *adv,
                  const int32_t *n_states, int64_t C, int Smax, const double *x, const int32_t *len, int64_t N,
                  int T, int F, double *score, int32_t *label, void *workspace, size_t workspace_bytes,
                  void *stream);
int dsp_hmm_align(const double *mu, const double *w, const double *g, const double *stay, const double *adv,
                  const int32_t *n_states, int64_t C, int Smax, const double *x, const int32_t *len, int64_t N,
                  int T, int F, const int32_t *group_start, const int32_t *members, int64_t P, double *score,
                  int32_t *seg, void *workspace, size_t workspace_bytes, void *stream);
int dsp_hmm_accumulate(const double *mu_prev, const double *var_prev, const int32_t *n_states, int64_t C,
                       int Smax, const double *x, const int32_t *len, int64_t N, int T, int F,
                       const int32_t *group_start, const int32_t *members, int64_t P, const int32_t *seg,
                       const double *score, double var_floor, double *mean, double *var, int32_t *cnt,
                       int32_t *n_valid, double *total, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Vector-quantisation codebooks on the frame sequences: the nearest codeword of every frame, the total
 * distortion of a sequence under a codebook, and one Lloyd re-estimation -- the pieces of LBG training
 * and of the VQ word recogniser (one codebook per word, the label of the smallest distortion).
 * csrc/vq.hip, DESIGN.md §4.13.  Every output is defined bit for bit: the device computes fp64 subtract,
 * multiply, add, compare and (in the re-estimation) one divide in the order below, each operation
 * rounded, no FMA; there is no certificate and no math library.
 *
 * Sequences: x float64 [N, T, F] padded row-major with len int32 [N], 1 <= F <= 8, 1 <= T <= 1024 (the
 *   DTW plan above).
 * Codebook set: C <= 2^20 codebooks padded to Kmax <= 256 codewords: cb float64 [C, Kmax, F], n_codes
 *   int32 [C], 1 <= n_codes[c] <= Kmax.  Frames and codewords are finite; for other values the results
 *   are unspecified, but nothing is read or written out of bounds.  Rows k >= n_codes[c] are never read
 *   by the search.
 * For frame t of a sequence of n frames and a codebook of K codewords:
 *     d(t,k) = e0 * e0, then for f = 1 .. F-1 ascending:  e = x[t,f] - cb[k,f];  d = d + e * e
 *                                                         (e0 = x[t,0] - cb[k,0])
 *     best = d(t,0), code = 0;  for k = 1 .. K-1 ascending:  if d(t,k) < best (strictly): best = d(t,k), code = k
 *     D = best(0);  D = D + best(t)  for t = 1 .. n-1 ascending
 *   Ties go to the smaller codeword index; D is the sequence's total distortion.  D is +inf, and every
 *   code -1, when n < 1, n > T, n_codes[c] is outside 1 .. Kmax, or a list entry is outside [0, N);
 *   nothing of such a member is read through.  A distance that overflows is +inf; if all overflow the
 *   code is 0.
 * Pairs (dsp_vq_assign, dsp_vq_accumulate): dsp_dtw_align's CSR list over the codebooks -- group_start
 *   int32 [C + 1], members int32 [P]; a sequence may appear under several codebooks and several times
 *   under one; a group may be empty.
 *
 * dsp_vq_score: every sequence against every codebook, score float64 [N, C] (= D); label int32 [N] the
 *   codebook of the smallest D, ties to the smaller index, -1 when every D is +inf.  Either output may
 *   be NULL.
 * dsp_vq_assign: dist float64 [P] (= D) and code int32 [P, T] of the listed pairs: code[p, t] is the
 *   frame's codeword, -1 for t >= n and everywhere for an invalid pair.  Either may be NULL (without
 *   code nothing per frame is stored).
 * dsp_vq_accumulate: one Lloyd re-estimation of every codebook from a GIVEN code [P, T] and dist [P]
 *   (the output of dsp_vq_assign, or the caller's own, e.g. all zeros for the one-codeword start).  A
 *   member is valid when its index and length are and every code[p, t], t < n, lies in [0, n_codes[c]);
 *   other members are skipped and nothing of their frames is read.  For codebook c with valid members
 *   k0 < k1 < ... in list order:
 *     m_k[j]    = number of the member's frames with code j
 *     X_k[j,f]  = the member's frames with code j added left to right (t ascending; the first is the
 *                 value itself)
 *     accX[j,f] = X_k of the first member with m_k[j] > 0, then accX + X_k for each later member with
 *                 m_k[j] > 0, in list order (a member with m_k[j] = 0 adds nothing to cell j -- not even
 *                 0.0, so a cell of -0.0 frames stays -0.0)
 *     cnt[j]    = sum_k m_k[j]                          integer
 *     centroid[j,f] = accX[j,f] / (double) cnt[j] where cnt[j] > 0;  cb_prev[c,j,f] bit for bit where not
 *     total[c]  = dist_k0 + dist_k1 + ...               in list order;  n_valid[c] = number of valid members
 *   Outputs centroid float64 [C, Kmax, F] (may not be cb_prev), cnt int32 [C, Kmax], n_valid int32 [C],
 *   total float64 [C].  Rows j >= K are zeros.  A codebook with no valid member or an n_codes outside
 *   1 .. Kmax is copied bit for bit from cb_prev (all Kmax rows), with total 0.0, n_valid 0 and cnt 0.
 * workspace  device scratch of dsp_vq_workspace_bytes(C, N, P, T, F, Kmax) bytes (0: sizes outside the
 *   plan; P = 0 for dsp_vq_score): N x C scores (labels without scores), and for the re-estimation the
 *   sums, counts and validity of one chunk of pairs (at most 128 MiB) and the codebooks' counts.
 *   Nothing in it is carried from one call to the next.
 * All three check their host arguments before any launch (DSP_ERR_ARGS, DSP_ERR_WORKSPACE), return
 * DSP_OK with nothing to do, make no host synchronisation and no allocation, and write only to their
 * outputs and the workspace, on the caller's stream.
 */
size_t dsp_vq_workspace_bytes(int64_t C, int64_t N, int64_t P, int T, int F, int Kmax);
int dsp_vq_score(const double *cb, const int32_t *n_codes, int64_t C, int Kmax, const double *x,
                 const int32_t *len, int64_t N, int T, int F, double *score, int32_t *label, void *workspace,
                 size_t workspace_bytes, void *stream);
int dsp_vq_assign(const double *cb, const int32_t *n_codes, int64_t C, int Kmax, const double *x,
                  const int32_t *len, int64_t N, int T, int F, const int32_t *group_start,
                  const int32_t *members, int64_t P, double *dist, int32_t *code, void *workspace,
                  size_t workspace_bytes, void *stream);
int dsp_vq_accumulate(const double *cb_prev, const int32_t *n_codes, int64_t C, int Kmax, const double *x,
                      const int32_t *len, int64_t N, int T, int F, const int32_t *group_start,
                      const int32_t *members, int64_t P, const int32_t *code, const double *dist,
                      double *centroid, int32_t *cnt, int32_t *n_valid, double *total, void *workspace,
                      size_t workspace_bytes, void *stream);

/*
 * Left-to-right hidden Markov models with DISCRETE observations: the frames are quantised once against
 * one shared codebook (dsp_vq_assign with members = 0 .. N-1 of one group is the tokeniser) and every
 * state emits symbols with a probability table.  csrc/dhmm.hip, DESIGN.md §4.14.  An extension like the
 * entry points above from dsp_dtw_* on: nothing here restates a reference file.  Every output is defined
 * bit for bit: the device computes fp64 add and min in the order below, each operation rounded, and
 * integer counts; the logarithms are the caller's, taken when the model is built.
 *
 * Symbols: sym int32 [N, T] padded row-major with len int32 [N], 1 <= T <= 1024 -- the layout of
 *   dsp_vq_assign's code.  Entries at t >= len are never read through, whatever they hold.
 * Alphabet: K symbols, 1 <= K <= 256, shared by all models of a set.
 * Model set: C <= 2^20 models padded to Smax states, 1 <= n_states[c] <= Smax <= 32: emit float64
 *   [C, Smax, K] (= -log b_s(k)), stay, adv float64 [C, Smax], n_states int32 [C].  All finite or +inf,
 *   never NaN, never -inf; adv[c, S-1] and the rows s >= S are never read.
 * Recurrence, for a sequence of length n and a model of S states:
 *     e(t,s) = emit[c, s, sym[t]]
 *     V(0,0) = e(0,0);  V(0,s>0) = +inf
 *     a = V(t-1,s) + stay[s];  b = V(t-1,s-1) + adv[s-1]        (b = +inf at s = 0)
 *     V(t,s) = e(t,s) + min(a, b)
 *     score  = V(n-1, S-1)
 *   score is +inf when n < S, when n < 1 or n > T, when n_states[c] is outside 1 .. Smax, for a list
 *   entry outside [0, N), and when any sym[t], t < n, lies outside [0, K) (such a symbol never indexes
 *   the table).
 * Path, seg int32 [P, Smax] and the -1 rules: dsp_hmm_align's above, word for word (advance iff b < a).
 * Pairs (dsp_dhmm_align, dsp_dhmm_accumulate): dsp_dtw_align's CSR list over the models.
 *
 * dsp_dhmm_score: every sequence against every model, score float64 [N, C]; label int32 [N] the model of
 *   the smallest score, ties to the smaller index, -1 when every score is +inf.  Either may be NULL.
 * dsp_dhmm_align: score float64 [P] and seg int32 [P, Smax] of the listed pairs; either may be NULL
 *   (without seg no direction bit is stored and no path is walked).
 * dsp_dhmm_accumulate: the Viterbi re-estimate from a GIVEN seg [P, Smax] and score [P].  A member is
 *   valid when its index and length are, its seg row is well formed for its model (seg[0] = 0, strictly
 *   increasing over the S states, seg[S-1] < n) and every sym[t], t < n, lies in [0, K); any other member
 *   is skipped whole.  Outputs:
 *     cnt_emit int32 [C, Smax, K]  frames of valid members that sit in state s and carry symbol k
 *     cnt      int32 [C, Smax]     frames of valid members in state s
 *     n_valid  int32 [C]           valid members
 *     total    float64 [C]         their scores added in list order, the first being the value itself
 *   Rows s >= S are zeros.  A model with no valid member or an n_states outside 1 .. Smax has all-zero
 *   counts, total 0.0 and n_valid 0.
 * workspace  device scratch of dsp_dhmm_workspace_bytes(C, N, P, T, Smax, K) bytes (0: sizes outside the
 *   plan; P = 0 for dsp_dhmm_score): the model set repacked (emission tables transposed to one row per
 *   symbol), one 32-bit direction word per row and lane for each resident wave (at most 256 MiB), N x C
 *   scores (labels without scores), and one int32 per pair for the re-estimation.  Nothing in it is
 *   carried from one call to the next.
 * All three check their host arguments before any launch (DSP_ERR_ARGS, DSP_ERR_WORKSPACE), return
 * DSP_OK with nothing to do, make no host synchronisation and no allocation, and write only to their
 * outputs and the workspace, on the caller's stream.
 */
size_t dsp_dhmm_workspace_bytes(int64_t C, int64_t N, int64_t P, int T, int Smax, int K);
int dsp_dhmm_score(const double *emit, const double *stay, const double *adv, const int32_t *n_states, int64_t C,
                   int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N, int T, double *score,
                   int32_t *label, void *workspace, size_t workspace_bytes, void *stream);
int dsp_dhmm_align(const double *emit, const double *stay, const double *adv, const int32_t *n_states, int64_t C,
                   int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N, int T,
                   const int32_t *group_start, const int32_t *members, int64_t P, double *score, int32_t *seg,
                   void *workspace, size_t workspace_bytes, void *stream);
int dsp_dhmm_accumulate(const int32_t *n_states, int64_t C, int Smax, int K, const int32_t *sym, const int32_t *len,
                        int64_t N, int T, const int32_t *group_start, const int32_t *members, int64_t P,
                        const int32_t *seg, const double *score, int32_t *cnt_emit, int32_t *cnt, int32_t *n_valid,
                        double *total, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Forward scoring (evaluation) and forward-backward expected counts (Baum-Welch training) of the
 * discrete-observation HMMs above, in the SCALED PROBABILITY domain.  csrc/dhmm_fb.hip, DESIGN.md §4.16.
 * Every row of the trellis is rescaled by a power of two taken from the row's own maximum, so the device
 * needs only fp64 multiply, add, max, frexp and ldexp and one IEEE division per frame.  Every output is
 * defined bit for bit; the device takes no logarithm: the likelihood leaves it as a (mantissa, exponent)
 * pair and the caller takes the one log.
 *
 * Symbols: sym int32 [N, T] with len int32 [N], 1 <= T <= 1024, as in dsp_dhmm_score.  Alphabet: K <= 256.
 * Probability model set: C <= 2^20 models padded to Smax <= 32 states: pemit float64 [C, Smax, K], pstay,
 *   padv float64 [C, Smax], n_states int32 [C].  Every entry read is either 0.0 or lies in [2^-300, 1],
 *   never NaN; padv[c, S-1] and the rows s >= S are never read.
 * Arithmetic: every operation is rounded to fp64, products are formed as written, nothing is fused, fp64
 *   denormals are kept.  Below B = pemit, a = pstay, d = padv, o = the symbol row.
 * Forward, for a model of S states and a sequence of n frames:
 *     u_0(0) = B[0,o_0];   u_0(s>0) = 0
 *     u_t(s) = (A_{t-1}(s)*a[s] + A_{t-1}(s-1)*d[s-1]) * B[s,o_t]   (the second product is 0.0 at s = 0)
 *     m_t = max_s u_t(s)
 *       m_t > 0:  k_t = frexp exponent of m_t  (m_t = f * 2^k_t, 0.5 <= f < 1)
 *                 A_t(s) = ldexp(u_t(s), -k_t);   E_t = E_{t-1} + k_t     (E_{-1} = 0)
 *       m_t == 0: A_t = u_t (all zeros);  E_t = E_{t-1}
 *     result:  v = A_{n-1}(S-1)
 *       v == 0:  (mant, expo) = (0.0, 0), "zero likelihood"
 *       else:    (f, k) = frexp(v);  mant = f in [0.5, 1);  expo = E_{n-1} + k     (int32)
 *   The likelihood of ending in the last state is mant * 2^expo.  It is zero when n < S (this comes out of
 *   the recurrence), when n < 1 or n > T, when n_states[c] is outside 1 .. Smax, for a list entry outside
 *   [0, N), and when any sym[t], t < n, lies outside [0, K) (such a symbol never indexes the table).
 *   Label: the model with the largest likelihood, decided exactly: the larger expo wins, then the larger
 *   mant, ties go to the smaller index; -1 when every model's likelihood is zero.
 * Backward:
 *     Bh_{n-1}(S-1) = 1;   Bh_{n-1}(s < S-1) = 0
 *     w_t(s) = a[s]*(B[s,o_{t+1}]*Bh_{t+1}(s)) + d[s]*(B[s+1,o_{t+1}]*Bh_{t+1}(s+1))   (second term 0.0 at s = S-1)
 *   Each row is rescaled by its own maximum's exponent exactly as above; a zero row stays zero.  No exponent
 *   is kept: the per-frame normalisation below cancels it.
 * Posteriors:
 *     g_t(s) = A_t(s) * Bh_t(s)
 *     D_t    = g_t(0) + g_t(1) + ... + g_t(S-1)    (ascending s)
 *     r_t    = 1.0 / D_t                           (one IEEE division per frame)
 *     gamma_t(s) = g_t(s) * r_t
 *   A member is valid when its index and length are valid, all its symbols at t < n lie in [0, K), its
 *   model's n_states is valid and every D_t, 0 <= t < n, is > 0 (D_{n-1} > 0 is the forward result being
 *   non-zero) and has a finite reciprocal r_t: a positive D_t below about 2^-1024 (a subnormal) gives
 *   r_t = +inf and makes the member invalid like D_t == 0, so no +inf and no 0 x inf is ever formed and
 *   gamma, occ_emit and n_valid hold finite values only.  Any other member is skipped whole.
 * Expected counts, for a valid pair p of model c:
 *     G_p[s,k]        the sum of gamma_t(s) over the frames with o_t = k, added in DESCENDING t from 0.0
 *     occ_emit[c,s,k] the G_p[s,k] of the valid members added in list order, starting from 0.0
 *     n_valid[c]      the valid members
 *   Rows s >= S are zeros; models without a valid member are zeros.  No transition counts are needed: in a
 *   left-to-right model without skips every path leaves each state s < S-1 exactly once, so the expected
 *   advance count of a state is n_valid and the expected stay count is its occupancy minus n_valid.
 *
 * dsp_dhmm_forward: every sequence against every model: mant float64 [N, C], expo int32 [N, C], label
 *   int32 [N].  Each may be NULL (a label without mant or expo keeps them in the workspace).
 * dsp_dhmm_expect: over dsp_dhmm_align's CSR pair list: mant float64 [P], expo int32 [P] and gamma float64
 *   [P, T, Smax], each of which may be NULL, and occ_emit float64 [C, Smax, K], n_valid int32 [C].  gamma is
 *   written at t < n and s < S for valid members; every other entry of gamma is 0.0.  mant and expo are
 *   written for the pairs inside a group (group_start[0] <= p < group_start[C]); entries of pairs outside
 *   every group are left as the caller had them.
 * workspace  device scratch of dsp_dhmm_fb_workspace_bytes(C, N, P, T, Smax, K) bytes (0: sizes outside the
 *   plan; P = 0 for dsp_dhmm_forward): the model set repacked, the scaled forward rows of each resident wave
 *   (at most 256 MiB; this caps the waves), one table G_p per pair of a pair chunk (at most 256 MiB; the
 *   list is processed in such chunks), one int32 per pair, and N x C (mant, expo) for labels without them.
 *   Nothing in it is carried from one call to the next.
 * Both check their host arguments before any launch (DSP_ERR_ARGS, DSP_ERR_WORKSPACE), return DSP_OK with
 * nothing to do, make no host synchronisation and no allocation, and write only to their outputs and the
 * workspace, on the caller's stream.
 */
size_t dsp_dhmm_fb_workspace_bytes(int64_t C, int64_t N, int64_t P, int T, int Smax, int K);
int dsp_dhmm_forward(const double *pemit, const double *pstay, const double *padv, const int32_t *n_states, int64_t C,
                     int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N, int T, double *mant,
                     int32_t *expo, int32_t *label, void *workspace, size_t workspace_bytes, void *stream);
int dsp_dhmm_expect(const double *pemit, const double *pstay, const double *padv, const int32_t *n_states, int64_t C,
                    int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N, int T,
                    const int32_t *group_start, const int32_t *members, int64_t P, double *mant, int32_t *expo,
                    double *gamma, double *occ_emit, int32_t *n_valid, void *workspace, size_t workspace_bytes,
                    void *stream);

/*
 * Connected-word decoding: the one-pass (token-passing) Viterbi over a loop of the word models of a
 * dsp_dhmm_* set.  An utterance holds several words in a row with unknown boundaries; the result is the
 * word sequence.  csrc/dhmm_decode.hip, DESIGN.md §4.15.  Bit for bit like the entry points above: fp64
 * add and compare only, each operation rounded.
 *
 * Inputs.  The model set of dsp_dhmm_score with the same value rules: emit float64 [C, Smax, K], stay,
 *   adv float64 [C, Smax], n_states int32 [C]; adv[c, S-1] stays unread: leaving a word's last state is
 *   free.  enter float64 [C] is the cost of starting word c (a word penalty plus, if the caller wants,
 *   -log of a prior): finite or +inf, never NaN, never -inf; NULL means all 0.0.  A model with
 *   n_states[c] outside 1 .. Smax counts as enter[c] = +inf: it is never entered and never read.
 *   1 <= C <= 64 (DSP_DHMM_DECODE_MAX_MODELS), Smax <= 32, K <= 256.  sym int32 [N, T], len int32 [N],
 *   T <= 1024, as for dsp_dhmm_score.
 * Recurrence.  For an utterance of n frames every cell is (V, start), with V(-1, ., .) = +inf and
 *   X(-1) = 0.0.  For t = 0 .. n-1, model c with S = n_states[c], state s:
 *     e = emit[c, s, sym[t]]
 *     a = V(t-1,c,s) + stay[c,s]
 *     b = s > 0 ?  V(t-1,c,s-1) + adv[c,s-1]  :  X(t-1) + enter[c]
 *     advance iff b < a (strictly; ties stay)
 *     V(t,c,s)     = e + (advance ? b : a)
 *     start(t,c,s) = advance ? (s > 0 ? start(t-1,c,s-1) : t) : start(t-1,c,s)
 *     X(t) = min over c ascending of V(t,c,S_c-1), a later c replacing only if strictly smaller
 *     W(t) = that c (-1 when every exit is +inf)
 *     B(t) = start(t, W(t), S_W-1)
 * Result.  score = X(n-1).  The words are walked back: t = n-1; the word is W(t) and it starts at B(t);
 *   then t = B(t) - 1, until t < 0.  Outputs, in time order:
 *     score    float64 [N]             X(n-1)
 *     n_words  int32 [N]               the true number of words
 *     words    int32 [N, max_words]    the word models in time order
 *     start    int32 [N, max_words]    first frame of each word
 *     cum      float64 [N, max_words]  X at each word's last frame, so the last one is score
 *   With more than max_words words the first max_words in time order are written; 1 <= max_words <= T.
 *   Entries behind the words are -1 (cum: +inf).  score is +inf, n_words 0 and the rows -1 / +inf when
 *   n < 1 or n > T, when any sym[t], t < n, lies outside [0, K) (such a symbol never indexes a table), and
 *   when no word can end at n-1.  Any output may be NULL.
 * workspace  device scratch of dsp_dhmm_decode_workspace_bytes(C, N, T, Smax, K) bytes (0: sizes outside
 *   the plan): the set transposed to one 512-byte line per (symbol, state slot) across the 64 models, the
 *   transitions and entry costs per slot.  Nothing in it is carried from one call to the next.
 * dsp_dhmm_decode checks its host arguments before any launch (DSP_ERR_ARGS, DSP_ERR_WORKSPACE), returns
 * DSP_OK with nothing to do (N = 0, every output NULL), makes no host synchronisation and no allocation,
 * and writes only to its outputs and the workspace, on the caller's stream.
 */
#define DSP_DHMM_DECODE_MAX_MODELS 64
size_t dsp_dhmm_decode_workspace_bytes(int64_t C, int64_t N, int T, int Smax, int K);
int dsp_dhmm_decode(const double *emit, const double *stay, const double *adv, const int32_t *n_states,
                    const double *enter, int64_t C, int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N,
                    int T, int max_words, double *score, int32_t *n_words, int32_t *words, int32_t *start, double *cum,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Connected-word decoding under a word-pair grammar: dsp_dhmm_decode's one-pass Viterbi with the cost of a
 * word change depending on the word before -- a bigram over the words, or a finite-state syntax ("after
 * open only door or window") as 0.0 / +inf costs.  csrc/dhmm_grammar.hip, DESIGN.md §4.19.  Bit for bit
 * like the entry points above: fp64 add and compare only, each operation rounded.
 *
 * Inputs.  The model set, sym, len, N, T and max_words are those of dsp_dhmm_decode, with the same value
 *   rules and bounds: 1 <= C <= 64, Smax <= 32, K <= 256, T <= 1024.
 *     enter  float64 [C]     the cost of STARTING THE UTTERANCE with word c; NULL means all 0.0
 *     pair   float64 [C, C]  row-major: pair[p, c] is the cost of word c following word p; required; it
 *                            carries everything a word change costs, any word penalty included
 *     leave  float64 [C]     the cost of ending the utterance on word c; NULL means all 0.0
 *   All three are finite or +inf, never NaN, never -inf; +inf forbids.  A model with n_states outside
 *   1 .. Smax is neither a predecessor nor a successor and is never read; the cost rows and columns of such
 *   a model may hold anything.
 * Recurrence.  The cells are dsp_dhmm_decode's: the value (advance ? b : a) is selected by the same strict
 *   compare that moves start, and ties stay.  Only the entry term of state 0 changes:
 *     G(-1, c) = 0.0 + enter[c];   P(-1, c) = -1
 *     b at s = 0 of frame t:  G(t-1, c)                      (was X(t-1) + enter[c])
 *     E(t, p) = V(t, p, S_p - 1);   Bx(t, p) = start(t, p, S_p - 1)
 *     G(t, c) = min over valid p ascending of  E(t, p) + pair[p, c],
 *               a later p replacing only if strictly smaller;  P(t, c) = that p (-1 when all are +inf)
 *     score   = min over valid c ascending of  E(n-1, c) + leave[c], same tie rule;  w = that c
 * Walk back.  Start at t = n-1 with word w.  It starts at b = Bx(t, w).  If b = 0, stop.  Otherwise the
 *   word before it is P(b-1, w), ending at frame b-1; repeat from there.
 * Outputs, in time order: score float64 [N], n_words int32 [N] (the true number), words and start int32
 *   [N, max_words].  The first max_words words are written, with -1 behind them.  The forced rows are
 *   dsp_dhmm_decode's: score +inf, n_words 0 and -1 rows when n < 1 or n > T, when any sym[t], t < n, lies
 *   outside [0, K), and when no score is finite.  Any output may be NULL.  There is no cum output: it would
 *   need every lane's exit value per frame kept as well.
 * workspace  device scratch of dsp_dhmm_decode_grammar_workspace_bytes(C, N, T, Smax, K) bytes (0: sizes
 *   outside the plan): dsp_dhmm_decode's transposed set and one 32-bit word per frame and model for each
 *   utterance in flight.  Nothing in it is carried from one call to the next.
 * dsp_dhmm_decode_grammar checks its host arguments before any launch (DSP_ERR_ARGS, DSP_ERR_WORKSPACE),
 * returns DSP_OK with nothing to do (N = 0, every output NULL), makes no host synchronisation and no
 * allocation, and writes only to its outputs and the workspace, on the caller's stream.
 */
size_t dsp_dhmm_decode_grammar_workspace_bytes(int64_t C, int64_t N, int T, int Smax, int K);
int dsp_dhmm_decode_grammar(const double *emit, const double *stay, const double *adv, const int32_t *n_states,
                            const double *enter, const double *pair, const double *leave, int64_t C, int Smax, int K,
                            const int32_t *sym, const int32_t *len, int64_t N, int T, int max_words, double *score,
                            int32_t *n_words, int32_t *words, int32_t *start, void *workspace, size_t workspace_bytes,
                            void *stream);

/*
 * Forced alignment and embedded Viterbi re-estimation: an utterance of several words in a row with a KNOWN
 * word sequence (its transcript) is aligned against the concatenation of the transcript's word models, and
 * the models are re-estimated from those alignments -- training on the kind of data dsp_dhmm_decode decodes,
 * with no word boundary marked by hand.  csrc/dhmm_force.hip, DESIGN.md §4.18.  Bit for bit like the entry
 * points above: fp64 add and compare and integer counts only.
 *
 * Inputs.  The model set and enter float64 [C] exactly as for dsp_dhmm_decode, with the same value rules;
 *   enter NULL means all 0.0.  1 <= C <= 64, Smax <= 32, K <= 256.  sym int32 [N, T], len int32 [N],
 *   T <= 1024.  trans int32 [N, Wmax]: the model index of each word of utterance u's transcript, in time
 *   order; n_trans int32 [N] its word count; 1 <= Wmax <= 64 (DSP_DHMM_FORCE_MAX_WORDS).  Entries of trans
 *   behind n_trans[u] are never read through.
 * Recurrence.  Utterance u of n frames with transcript w_0 .. w_{L-1}, S_i = n_states[w_i]; position i has
 *   the states (i, 0 .. S_i - 1); V(-1, ., .) = +inf.  For t = 0 .. n-1:
 *     e = emit[w_i, s, sym[t]]
 *     a = V(t-1,i,s) + stay[w_i,s]
 *     b = s > 0   ?  V(t-1,i,s-1) + adv[w_i,s-1]
 *       : i > 0   ?  V(t-1,i-1,S_{i-1}-1) + enter[w_i]
 *       : t == 0  ?  0.0 + enter[w_0]
 *       :            +inf
 *     advance iff b < a (strictly; ties stay)
 *     V(t,i,s) = e + (advance ? b : a)
 *     score = V(n-1, L-1, S_{L-1}-1)
 *   This is dsp_dhmm_decode's cell with the word loop replaced by the transcript's chain; the decoder's
 *   free exit is kept: adv[c, S-1] stays unread.
 * Result.  score float64 [N].  seg int32 [N, Wmax, Smax]: the first frame of every state of every position,
 *   an absolute frame index of the utterance, walked back from (n-1, L-1, last state) along the advance
 *   decisions; -1 for s >= S_i and for i >= L.  seg[u, i, 0] is word i's first frame.
 *   score is +inf and the whole seg row -1 when n < 1 or n > T; when L < 1 or L > Wmax; when some
 *   trans[u, i], i < L, lies outside [0, C) or names a model whose n_states is outside 1 .. Smax; when some
 *   sym[t], t < n, lies outside [0, K) (such a symbol never indexes a table); and when the recurrence leaves
 *   +inf (n < sum S_i, a +inf enter, ...).  Either output may be NULL; without seg no direction bit is
 *   stored and nothing is walked.
 * dsp_dhmm_force_accumulate: the embedded Viterbi re-estimate from a GIVEN seg [N, Wmax, Smax], as
 *   dsp_dhmm_accumulate is from its seg.  An utterance is valid when its length and its transcript are valid
 *   as above, all its symbols are in range and its seg row is well formed: seg[0][0] = 0, strictly increasing
 *   over the sum S_i concatenated states, the last one < n, and -1 exactly where the definition says.  Any
 *   other utterance is skipped whole, with valid[u] = 0.
 *     cnt_emit int32 [C, Smax, K]  frames of valid utterances that sit in state s of an instance of word c
 *                                  and carry symbol k
 *     cnt      int32 [C, Smax]     frames of valid utterances in state s of an instance of word c
 *     n_valid  int32 [C]           word instances of c in valid utterances: every instance leaves each of its
 *                                  states once, so p_stay = (cnt - n_valid) / cnt as for dsp_dhmm_accumulate
 *     valid    int32 [N]           1 for a valid utterance, 0 for a skipped one
 *   Rows s >= S are zero, as is a model with no instance.  All counts are integers, gathered with integer
 *   atomics in any order and still defined exactly; the call zeroes them itself.  No floating-point total is
 *   formed on the device: the training objective is the caller's, from dsp_dhmm_force_align's scores.
 * workspace  device scratch of dsp_dhmm_force_workspace_bytes(C, N, T, Wmax, Smax, K) bytes (0: sizes outside
 *   the plan) for either call: dsp_dhmm_decode's transposed set and one 32-bit direction word per frame and
 *   lane of every resident wave.  Nothing in it is carried from one call to the next.
 * Both calls check their host arguments before any launch (DSP_ERR_ARGS, DSP_ERR_WORKSPACE), return DSP_OK
 * with nothing to do (dsp_dhmm_force_align: N = 0 or both outputs NULL; dsp_dhmm_force_accumulate with N = 0
 * zeroes the counts), make no host synchronisation and no allocation, and write only to their outputs and the
 * workspace, on the caller's stream.
 */
#define DSP_DHMM_FORCE_MAX_WORDS 64
size_t dsp_dhmm_force_workspace_bytes(int64_t C, int64_t N, int T, int Wmax, int Smax, int K);
int dsp_dhmm_force_align(const double *emit, const double *stay, const double *adv, const int32_t *n_states,
                         const double *enter, int64_t C, int Smax, int K, const int32_t *sym, const int32_t *len, int64_t N,
                         int T, const int32_t *trans, const int32_t *n_trans, int Wmax, double *score, int32_t *seg,
                         void *workspace, size_t workspace_bytes, void *stream);
int dsp_dhmm_force_accumulate(const int32_t *n_states, int64_t C, int Smax, int K, const int32_t *sym, const int32_t *len,
                              int64_t N, int T, const int32_t *trans, const int32_t *n_trans, int Wmax, const int32_t *seg,
                              int32_t *cnt_emit, int32_t *cnt, int32_t *n_valid, int32_t *valid, void *workspace,
                              size_t workspace_bytes, void *stream);

/*
 * Short-time autocorrelation pitch track -- the fourth classical time-domain feature next to energy,
 * magnitude and ZCR, on the crop frames that dsp_extract_features found.  csrc/pitch.hip, DESIGN.md
 * §4.11.  Every output is an exact integer; no floating point is involved.
 *
 * A clip is x[0..N) int16, its crop [st, en) and its frame count nf as dsp_extract_features wrote
 * them, L = frame_length, S = frame_shift, 1 <= lag_min <= lag_max <= L - 1.
 *   centring  c = floor((2 sum(x) + N) / (2 N))   the clip mean rounded half up, exact integers
 *             y[n] = x[n] - c                     |y| <= 65535
 *   frames    t = 0 .. nf - 1, frame_signal's frames, the last one zero-padded, no window:
 *             f_t[i] = y[st + t S + i] if st + t S + i < en, else 0      0 <= i < L
 *   r_t(tau)  = sum_{i=0}^{L-1-tau} f_t[i] f_t[i + tau]                  exact int64
 *   lag[t]    the SMALLEST tau in [lag_min, lag_max] that maximises r_t(tau)
 *   peak[t]   r_t(lag[t])
 *   r0[t]     r_t(0)
 * All three are written for every frame, voiced or not; an all-zero frame gives lag_min, 0, 0.
 * Voicing and f0 are pure functions of these and are the caller's:
 *   voiced = peak > 0 and vden * peak >= vnum * r0 (int64; 1 <= vnum <= vden <= 1024, default 3/10),
 *   f0 = sample_rate / lag (one fp64 division), 0.0 where unvoiced.
 *
 * pcm, offsets  as dsp_extract_features (pcm 4-byte aligned is enough here).
 * start_end, n_frames, status  that call's outputs, read on the device; out_stride as there (0: separate
 *             arrays; 19: the packed rows pass straight in as rows + 15, rows + 17, rows + 18).
 * lag int32, peak int64, r0 int64  [B, ld].  Frames t >= min(nf, ld) are left untouched, and so are the
 *             rows of clips with status & 0xFF != 0, of clips longer than max_len and of clips whose
 *             crop does not lie inside the clip (nothing is read outside a clip).
 * workspace   device scratch of dsp_pitch_workspace_bytes(...) bytes (0: outside the plan -- B >= 0,
 *             max_len >= 1, 2 <= L <= 4096, S >= 1, the lag range above); its first int32 is left
 *             holding the number of frames answered by the plain int64 path (frames with a sample
 *             y >= 32640 or y < -32896, whose high byte digit does not fit the i8 matrix cores).
 * Host checks before the launch (DSP_ERR_ARGS, DSP_ERR_WORKSPACE); B = 0 returns DSP_OK without a
 * launch; stream-ordered, no allocation, no copy, no synchronisation.
 */
size_t dsp_pitch_workspace_bytes(int B, int64_t max_len, int frame_length, int frame_shift, int lag_min,
                                 int lag_max);
int dsp_pitch_track(const int16_t *pcm, const int64_t *offsets, int B, int64_t max_len, int frame_length,
                    int frame_shift, int lag_min, int lag_max, const int32_t *start_end,
                    const int32_t *n_frames, const int32_t *status, int out_stride, int32_t *lag, int64_t *peak,
                    int64_t *r0, int ld, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Linear prediction of the crop frames -- the exact integer autocorrelation of each (windowed) frame,
 * then the Levinson-Durbin recursion and the LPC cepstrum in bit-defined fp64.  csrc/lpc.hip, DESIGN.md
 * §4.12.  Two entry points: dsp_lpc_autocorr (PCM -> r) and dsp_lpc_solve (r -> a, k, err, cepstrum).
 *
 * dsp_lpc_autocorr.  A clip, its crop [st, en), nf, L, S, the centring value c, y = x - c and the frames
 * f_t[i] are exactly dsp_pitch_track's (above).  p = order, 1 <= p <= min(32, L - 1).
 *   window    w[i] = min(max(window[i], 0), 32768)                       a Q15 table, 32768 = 1.0
 *             z_t[i] = (f_t[i] * w[i] + 16384) >> 15                      arithmetic shift (a floor):
 *             the product rounded half up back to an integer, |z| <= |y| <= 65535.  window == NULL means
 *             z = f, the same as every entry being 32768.
 *   r_t(tau)  = sum_{i=0}^{L-1-tau} z_t[i] z_t[i + tau],  tau = 0 .. p     exact int64, |r| < 2^45
 * r  int64 [B, ld, p + 1].  Frames t >= min(nf, ld) are left untouched, and so are the rows of clips with
 *             status & 0xFF != 0, of clips longer than max_len and of clips whose crop does not lie inside
 *             the clip (nothing is read outside a clip).
 * window      device, int32 [L], or NULL.
 * pcm, offsets, start_end, n_frames, status, out_stride, ld  as dsp_pitch_track.
 * workspace   device scratch of dsp_lpc_workspace_bytes(...) bytes (0: outside the plan -- B >= 0,
 *             max_len >= 1, 2 <= L <= 4096, S >= 1, 1 <= p <= min(32, L - 1)); its first int32 is left
 *             holding the number of frames answered by a plain fallback path, which is always 0: the lag
 *             sums run on the vector ALU for every frame and have no fallback.
 * Host checks before the launch (DSP_ERR_ARGS, DSP_ERR_WORKSPACE); B = 0 returns DSP_OK without a
 * launch; stream-ordered, no allocation, no copy, no synchronisation.
 *
 * dsp_lpc_solve.  r [n, p + 1] int64 (any values, a caller's own included), 1 <= p <= 32, 0 <= n < 2^31,
 * Q = n_cep, 0 <= Q <= 64.  Every operation below is one IEEE fp64 operation rounded to nearest even, in
 * this order, never fused; there is no log, exp or sqrt: convert, add, subtract, multiply, divide, compare.
 *   R[j] = (double) r[j]                      (round to nearest even; exact for |r| < 2^53)
 *   a[1..p] = k[1..p] = 0;  E = R[0];  m = 0
 *   for i = 1..p:
 *       if not (E > 0): stop
 *       acc = R[i];  for j = 1..i-1 ascending:  acc = acc - a[j] * R[i-j]
 *       ki = acc / E
 *       if not (|ki| < 1): stop               (also catches inf; no NaN can arise before it)
 *       for j = 1..i-1:  a'[j] = a[j] - ki * a[i-j];   a'[i] = ki;   a = a';   k[i] = ki
 *       E = E * (1 - ki * ki);   m = i
 *   err = E;  reached = m                     (the predictor is x^[n] = sum_j a_j x[n-j]; a_j = 0 for j > m)
 *   for n = 1..Q:
 *       s = 0;  for q = max(1, n-p) .. n-1 ascending:  s = s + ((double) q * c[q]) * a[n-q]
 *       c[n] = (n <= p ? a[n] : 0) + s / (double) n
 * With |ki| < 1 enforced every quantity stays finite: no output ever holds a NaN.  An all-zero row gives
 * reached = 0, err = 0 and zeros everywhere.  c[0] needs a logarithm and is the caller's.
 * a, k  fp64 [n, p] (a[row][j-1] = a_j);  err fp64 [n];  reached int32 [n];  cep fp64 [n, Q] (c_1 first),
 *             NULL exactly when Q = 0 is allowed (a NULL cep with Q > 0 is DSP_ERR_ARGS).
 * Host checks before the launch (DSP_ERR_ARGS); n = 0 returns DSP_OK without a launch; stream-ordered, no
 * allocation, no copy, no synchronisation, no workspace.
 */
size_t dsp_lpc_workspace_bytes(int B, int64_t max_len, int frame_length, int frame_shift, int order);
int dsp_lpc_autocorr(const int16_t *pcm, const int64_t *offsets, int B, int64_t max_len, int frame_length,
                     int frame_shift, int order, const int32_t *window, const int32_t *start_end,
                     const int32_t *n_frames, const int32_t *status, int out_stride, int64_t *r, int ld,
                     void *workspace, size_t workspace_bytes, void *stream);
int dsp_lpc_solve(const int64_t *r, int64_t n, int order, int n_cep, double *a, double *k, double *err,
                  int32_t *reached, double *cep, void *stream);

/*
 * Batch WAV reader -- host only (no GPU, no stream): the file side of load_wav
 * (src/audio_processing.py:9-46) for a whole file list, on n_threads native threads.
 * dsp_wav_scan walks each file's RIFF chunks ('fmt ' with WAVE_FORMAT_PCM before 'data', chunks
 * padded to even sizes, nframes = data bytes // frame bytes, the data fully present) and reports
 * kind[i] = DSP_WAV_S16_MONO or DSP_WAV_U8_MONO with nsamp[i] samples at byte data_off[i], or
 * DSP_WAV_OTHER (any other layout, stereo included, or an unreadable / malformed file: the
 * caller's own reader decodes it or reports the reference's error).  dsp_wav_read writes the
 * samples of every S16/U8 mono file with nsamp > 0 to dst + dst_off[i] (HOST memory, e.g. a pinned
 * staging buffer): int16 as stored, 8-bit as ((u8 - 128) mod 256) like load_wav's uint8
 * arithmetic (:31-34); a file that fails to read is turned into DSP_WAV_OTHER in kind[].
 * paths: NUL-terminated file names.  Returns DSP_OK or DSP_ERR_ARGS.
 */
#define DSP_WAV_OTHER 0
#define DSP_WAV_S16_MONO 1
#define DSP_WAV_U8_MONO 2
int dsp_wav_scan(const char *const *paths, int64_t n, int n_threads, int32_t *kind, int64_t *nsamp,
                 int64_t *data_off);
int dsp_wav_read(const char *const *paths, int64_t n, int n_threads, int32_t *kind, const int64_t *nsamp,
                 const int64_t *data_off, const int64_t *dst_off, int16_t *dst);

/* ABI version of the loaded library (DSP_ABI_VERSION). */
int dsp_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DSP_AUDIOREC_H */
