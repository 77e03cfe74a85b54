/*
 * catfish_hip.h -- C ABI of the MI355X-native homopolymer-calling forward pass.
 *
 * This is the drop-in boundary for ONE call of the reference:
 *
 *     confidences = self.sess.run(self.predictions,
 *                                 feed_dict={self.x: input_x, self.p_dropout: 1.0})
 *                                         (reference catfish/models/rnn_class.py:214-216)
 *
 * i.e. the whole TensorFlow graph built by ResNetRNN.network_layer
 * (catfish/models/resnet_class.py:17-25,44-82), RNN.network_layer
 * (catfish/models/rnn_class.py:165-175), RNN.output_layer (:178-183) and
 * RNN.compute_accuracy (:82-88, self.predictions = sigmoid(logits)).
 * The reference has no native code; the entry points below are what a cgo /
 * ctypes / N-API binding of that one call binds.  Plain pointers and sizes
 * only -- no torch / TensorFlow types.
 *
 * Weights enter a model on the host (cf_model_create: BN folded, matrices
 * re-tiled and uploaded) or, for an fp32 model, from a device flat parameter
 * vector (cf_model_load_params: the same folding and re-tiling as a gather
 * kernel on a stream, so a training loop can update the weights in place).
 *
 * Threading: one cf_model per device per host thread; cf_infer is
 * asynchronous on the given HIP stream and keeps no global state.
 * Errors: 0 = ok, negative = failure; cf_last_error() returns the message of
 * the calling thread's last failure.
 */
#ifndef CATFISH_HIP_H
#define CATFISH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF_OK 0
#define CF_ERR_INVALID -1     /* bad argument / unsupported geometry (Python raises ValueError) */
#define CF_ERR_HIP -2         /* a HIP runtime call failed */
#define CF_ERR_NOMEM -3
#define CF_ERR_IO -4          /* a file could not be opened / written (Python raises OSError); host entry points only */

#define CF_WINDOW 35          /* rnn_class.py:27 (self.window) */

/* Bumped whenever a signature or a struct of this header changes; cf_abi_version() returns the value the library was built
 * with, so a binding can refuse a stale libcatfish_hip.so instead of calling it with the wrong arguments. */
#define CF_ABI_VERSION 9

/* Arithmetic of the biGRU layers (the residual blocks, the hidden state, the gates'
 * sigmoid/tanh and all accumulation are fp32 in every mode). */
#define CF_PREC_FP32 0        /* exact fp32 MFMA (v_mfma_f32_16x16x4_f32); default            */
#define CF_PREC_BF16X3 1      /* operands split hi+lo bf16, 3 bf16 MFMAs per product (~2^-17); */
                              /* every geometry: the tuned kernels for 64 units / 32 channels  */
                              /* with residual blocks, the any-size kernels for all others     */
                              /* (plain RNN type included); also the convs there               */
#define CF_PREC_BF16 2        /* operands rounded to bf16 (BASELINE config 4)                 */

/* Hyper-parameters: the keys of ResNetRNN.txt parsed by
 * neural_network.retrieve_hyperparams (catfish/neural_network.py:37-67)
 * that shape the forward graph. */
typedef struct cf_hparams {
    int32_t layer_size;          /* GRU units per direction (rnn_class.py:16): a multiple of 16, at most 256.
                                    64 with layer_size_res 32 (the shipped checkpoint) runs on the tuned kernels,
                                    every other geometry on the any-size kernels (fp32 only)            */
    int32_t n_layers;            /* stacked bidirectional layers (rnn_class.py:17)   */
    int32_t layer_size_res;      /* conv channels (resnet_class.py:11)               */
    int32_t n_layers_res;        /* residual blocks (resnet_class.py:10); 0 = RNN    */
    int32_t window;              /* must be 35                                       */
    float bn_epsilon;            /* tf.layers.batch_normalization epsilon (1e-3)     */
    int64_t max_windows_per_pass;/* scratch capacity per slot; longer inputs are chunked */
    int32_t n_streams;           /* scratch slots + internal streams that overlap the
                                    sub-batches of one call (0 = default 1 = none)       */
    int32_t precision;           /* CF_PREC_*                                          */
    int32_t fuse_layers;         /* all biGRU layers in ONE launch with dynamic tile queues (fp32,
                                    n_layers <= 3): 0 = auto (only passes of >= 6 full-chip rounds,
                                    where it measures +5 %), 1 = always, -1 = never          */
} cf_hparams;

/* One conv1d + batch_normalization pair, TF layout
 * (resnet_class.py:60-61 / 64-65 / 69-70 / 74-75). */
typedef struct cf_conv_bn {
    const float* kernel;          /* [ksize, cin, layer_size_res] */
    const float* bias;            /* [layer_size_res] */
    const float* gamma;           /* [layer_size_res] */
    const float* beta;
    const float* moving_mean;
    const float* moving_variance;
    int32_t ksize;
    int32_t cin;
} cf_conv_bn;

/* tf.contrib.rnn.GRUCell variables of one direction of one layer
 * (rnn_class.py:146); kernel rows [0,cin) multiply x, rows [cin,cin+H) multiply h. */
typedef struct cf_gru_dir {
    const float* gates_kernel;     /* [cin + H, 2H]  columns [0,H) = r, [H,2H) = u */
    const float* gates_bias;       /* [2H] */
    const float* candidate_kernel; /* [cin + H, H] */
    const float* candidate_bias;   /* [H] */
    int32_t cin;
} cf_gru_dir;

/* All 74 inference tensors of the checkpoint, host pointers, TF layout. */
typedef struct cf_weights {
    const cf_conv_bn* conv;        /* 4 * n_layers_res entries, graph order:
                                      per block: shortcut, first, middle (k=3), last */
    const cf_gru_dir* gru;         /* 2 * n_layers entries: [layer][fw, bw] */
    const float* dense_kernel;     /* final_fully_connected/kernel [2H, 1] (rnn_class.py:179) */
    const float* dense_bias;       /* [1] */
} cf_weights;

typedef struct cf_model cf_model;

/* Replaces neural_network.load_network + RNN.restore_network
 * (catfish/neural_network.py:26-34, rnn_class.py:191-198): folds BN into the
 * convs, re-tiles every matrix into MFMA A-fragment order and uploads it. */
int cf_model_create(const cf_weights* w, const cf_hparams* hp, int device, cf_model** out);
void cf_model_destroy(cf_model* m);

/* Values in the flat parameter vector of this model's geometry: the checkpoint's inference tensors in the operator's
 * order (torch_ops.tensor_names, TF layouts, flattened) -- packed_weights without its 8-value header. */
int cf_model_param_floats(const cf_model* m, int64_t* n);
/* BN folding and re-tiling of `params` (device fp32, cf_model_param_floats values) into this model's own weight buffers,
 * on `stream`.  Afterwards the model computes exactly what a fresh cf_model_create of the same values computes.
 * The first call builds a gather map (host work, one allocation, one synchronous upload); every later call is two
 * kernel launches on `stream` -- no allocation, no copy, no synchronisation, so it can be captured in a graph.
 * fp32 models only: a model created with CF_PREC_BF16X3 or CF_PREC_BF16 gets CF_ERR_INVALID.  `params` must stay
 * unchanged until the launches have run; calls that overlap a cf_infer of the same model on another stream race. */
int cf_model_load_params(cf_model* m, const float* params, void* stream);

/* Replaces RNN.infer's sess.run (rnn_class.py:213-219).
 * x: device pointer, [n_windows, 35] fp32 (window-major, as reshape_input
 * produces, catfish/infer.py:108-124).  probs: device pointer,
 * [n_windows * 35] fp32 = sigmoid(logits), same order as the reference's
 * flattened output.  stream: hipStream_t (NULL = default stream). */
int cf_infer(cf_model* m, const float* x, int64_t n_windows, float* probs, void* stream);

/* Same with host buffers (synchronous; H2D / D2H included). */
int cf_infer_host(cf_model* m, const float* x, int64_t n_windows, float* probs);

/* The same two calls with the pre-sigmoid logits as a second output (``self.logits`` of
 * RNN.output_layer, catfish/models/rnn_class.py:178-183): the reference evaluates its validation
 * loss on the logits (tf.losses.sigmoid_cross_entropy, rnn_class.py:74-79,236-237), which the
 * saturated fp32 probabilities cannot reproduce.  probs or logits may be NULL (not both). */
int cf_infer_logits(cf_model* m, const float* x, int64_t n_windows, float* probs, float* logits, void* stream);
int cf_infer_host_logits(cf_model* m, const float* x, int64_t n_windows, float* probs, float* logits);

/* Sticky device-side error of earlier asynchronous launches on this model (today: a bounded wait of the
 * fused biGRU launch or of a biGRU hand-off that timed out, which invalidates that launch's results).  Call it after
 * synchronising the stream a cf_infer was queued on; CF_OK, or CF_ERR_HIP with the message in
 * cf_last_error().  cf_infer / cf_infer_host also refuse to run while it is set. */
int cf_check_error(cf_model* m);
/* Reset that flag after the caller has dropped the results of the failed launch: the model is usable again (a fused
 * launch re-initialises its queues and flags every time; the boundary flags of the grid-wide biGRU schedule, which are
 * zero between launches unless a wait timed out, are zeroed here: the call synchronises the device). */
int cf_clear_error(cf_model* m);

/* Launch-regime switch points of this model on its device, for callers and tests that need to know which
 * kernels a call of n_windows uses (all in windows):
 *   out[0] = CUs of the device
 *   out[1] = largest call whose biGRU x projection is hoisted onto the idle CUs (latency mode, fp32)
 *   out[2] = largest call served by the cooperative latency-mode biGRU kernels (fp32); larger calls use the
 *            throughput kernels (one wave per tile)
 *   out[3] = smallest call whose biGRU layers go out as ONE fused launch when fuse_layers = 0 (auto);
 *            0 when this model never fuses */
int cf_launch_regimes(const cf_model* m, int64_t out[4]);

/* Read-level post-processing on device, replacing class_from_threshold +
 * correct_short (catfish/infer.py:128-138,174-198).  Reads are packed back to
 * back INCLUDING their zero padding (infer.py:31-38): read r owns samples
 * [read_offsets[r], read_offsets[r+1]) of probs, of which the first
 * read_lengths[r] are real (the reference trims the padding at infer.py:47).
 * labels[i] = 1 iff probs[i] >= threshold and i lies in a positive run of
 * length >= min_run inside the real part of its read; padding gets 0.
 * read_offsets: device int64[n_reads + 1]; read_lengths: device int64[n_reads];
 * total_samples = read_offsets[n_reads] (passed by value so that the call
 * stays asynchronous); labels: device uint8[total_samples]. */
int cf_postprocess(cf_model* m, const float* probs, const int64_t* read_offsets,
                   const int64_t* read_lengths, int64_t n_reads, int64_t total_samples,
                   float threshold, int32_t min_run, uint8_t* labels, void* stream);

/* Run boundaries of the corrected labels on device (the run-length half of hp_in_pred,
 * catfish/infer.py:141-162).  labels: device uint8[total_samples] as written by cf_postprocess
 * (padding = 0, so runs never cross reads -- this call sees labels only: where a read is packed WITHOUT padding,
 * read_lengths[r] == read_offsets[r+1] - read_offsets[r], and its last sample and the next read's first are both positive,
 * they come out as one run; catfish/infer.py:31-36 pads every read by at least one sample, and cf_postprocess_spans, which
 * has the read table, cuts such runs at the boundary).  starts / ends: device int64[max_runs], receive the packed
 * positions of every run's first sample and one-past-last sample in arbitrary order (sort both
 * ascending: the k-th start pairs with the k-th end); counts: device uint64[2] = number of starts and
 * of ends found (may exceed max_runs, in which case the lists are truncated). */
int cf_spans(cf_model* m, const uint8_t* labels, int64_t total_samples, int64_t max_runs,
             int64_t* starts, int64_t* ends, uint64_t* counts, void* stream);

/* cf_postprocess and cf_spans as ONE launch: threshold, correct_short and the run boundaries of the corrected labels (catfish/infer.py:
 * 128-138, 174-198 and the run-length half of hp_in_pred, :141-162) straight from the probabilities.  Arguments as in the two calls;
 * labels may be NULL when only the run lists are wanted (then they are never written).  A run lies inside the real part of ITS read,
 * also when reads are packed without padding: adjacent positive runs of two such reads are two runs.  counts is zeroed by the call (on
 * the stream). */
int cf_postprocess_spans(cf_model* m, const float* probs, const int64_t* read_offsets, const int64_t* read_lengths, int64_t n_reads,
                         int64_t total_samples, float threshold, int32_t min_run, uint8_t* labels, int64_t max_runs,
                         int64_t* starts, int64_t* ends, uint64_t* counts, void* stream);

/* Per-call scores of the runs cf_postprocess_spans reports (csrc/span_scores.hpp; span_scores.span_scores_host is the definition).
 * starts / counts: what that call wrote (device; counts[0] = number of starts, read on the card, so the call stays asynchronous).
 * For every k < min(counts[0], max_runs), row k describes the run that begins at starts[k] -- the maximal streak of
 * probs >= threshold (float32 compare, NaN is false) from there inside the real part of its read:
 *   ends_paired  device int64 [max_runs]      one past the run's last sample
 *   sums         device double [max_runs][3]  sum of p, of x and of x * x over the run (float32 values widened to double); signal,
 *                the normalised samples the network saw (device float32 [total_samples]), may be NULL: then columns 1 and 2 are
 *                not written
 *   extremes     device float [max_runs][2]   smallest and largest p of the run
 * Rows at and above min(counts[0], max_runs) are left untouched.  A start that is negative, >= total_samples or outside the real
 * part of its read gets an empty row (end = start, zero sums, min = +inf, max = -inf) and is never dereferenced: the call is
 * memory-safe for any contents of starts.  One wave per run, a fixed reduction order: equal inputs give equal bits. */
int cf_span_scores(cf_model* m, const float* probs, const float* signal /* NULL: no level sums */,
                   const int64_t* read_offsets, const int64_t* read_lengths, int64_t n_reads, int64_t total_samples,
                   float threshold, const int64_t* starts, const uint64_t* counts, int64_t max_runs,
                   int64_t* ends_paired, double* sums /* [max_runs][3]: sum p, sum x, sum x * x */, float* extremes /* [max_runs][2] */,
                   void* stream);

/* Bridging (csrc/post_bridge_rule.hpp; infer.bridge_gaps is the definition): cf_postprocess_spans with one step more.  Inside the real
 * part of ONE read, a maximal run of samples below the threshold of at most max_gap samples, with a sample at or above the threshold
 * directly before it and directly after it, counts as above the threshold; then correct_short and the run lists as in
 * cf_postprocess_spans.  Samples that touch a read's first or last real sample are never filled, padding is never read as a one, and
 * nothing is bridged from one read into the next, also when reads are packed without padding.  max_gap == 0 is cf_postprocess_spans
 * itself (same launches).  Otherwise the pair must satisfy min_run >= 1, max_gap >= 0, min_run + max_gap <= 64 and labels (NULL is
 * fine) must be 16-byte aligned: anything else is CF_ERR_INVALID before any launch -- there is no slower route. */
int cf_postprocess_spans_bridged(cf_model* m, const float* probs, const int64_t* read_offsets, const int64_t* read_lengths,
                                 int64_t n_reads, int64_t total_samples, float threshold, int32_t max_gap, int32_t min_run,
                                 uint8_t* labels /* NULL ok */, int64_t max_runs /* 0: labels and counts only */, int64_t* starts,
                                 int64_t* ends, uint64_t* counts, void* stream);

/* cf_span_scores for runs given by labels: "the run continues" is labels[i] != 0 (device uint8 [total_samples], what
 * cf_postprocess_spans_bridged wrote) instead of probs[i] >= threshold, so the samples of a bridged gap belong to the run's sums and
 * extremes.  Same rows, same empty-row rule, same memory safety for any contents of starts, same fixed reduction order. */
int cf_span_scores_labels(cf_model* m, const float* probs, const float* signal /* NULL: no level sums */, const uint8_t* labels,
                          const int64_t* read_offsets, const int64_t* read_lengths, int64_t n_reads, int64_t total_samples,
                          const int64_t* starts, const uint64_t* counts, int64_t max_runs, int64_t* ends_paired, double* sums,
                          float* extremes, void* stream);

/* Signal ingest on device, replacing normalize_raw_signal + the padding / reshape of
 * infer_class_from_signal (catfish/infer.py:96-105, 31-43) for many reads at once.
 * dac: device int16, the reads' raw DAC samples back to back (after the leader trim of
 * process_signal, infer.py:87-90); dac_offsets: device int64[n_reads + 1] sample offsets into
 * dac; win_offsets: device int64[n_reads + 1] first window of every read in the packed output;
 * x_out: device fp32 [win_offsets[n_reads], 35], receives (raw - median) / median(|raw - median|)
 * followed by each read's zero padding.  Results are bit-identical to numpy's float64
 * normalisation cast to float32. */
int cf_normalize(cf_model* m, const int16_t* dac, const int64_t* dac_offsets,
                 const int64_t* win_offsets, int64_t n_reads, float* x_out, void* stream);

/* Pipeline tail on the HOST (no device work, no cf_model): what the reference's per-file loop does with the spans of a read
 * (catfish/catfish:57-82 and center_hp, :121-135) for many reads held as flat tables.  Read r owns rows
 * [bounds[r], bounds[r+1]) of a table; span_* = the [start - 11, end + 16] spans of infer_class_from_signal; lengths[r] =
 * its second return value.  Output: hp_* = the merged, centred chunks (reads without spans get none and are absent from the
 * reference's hp_dict), nonhp_* = the complement (reads without spans get the single row (0, length), which the reference
 * stores as [([(0, len), len])], catfish:82).  Quirks kept: the merged list aliases the span lists, spans are edited in
 * place, and `hp_positions[i - 1]` at i = 0 is the read's last span.
 * Capacities (rows): hp >= n_spans + n_reads, nonhp >= n_spans + 2 n_reads always suffice. */
int cf_chunks_from_spans(const int64_t* span_bounds, const int64_t* span_start, const int64_t* span_end,
                         const int64_t* lengths, int64_t n_reads, int64_t chunk_size,
                         int64_t* hp_bounds, int64_t* hp_start, int64_t* hp_end, int64_t hp_capacity,
                         int64_t* nonhp_bounds, int64_t* nonhp_start, int64_t* nonhp_end, int64_t nonhp_capacity);
/* The JSON members `"name": [[a, b], ...]` of such a table joined by ", " (json.dump's text between the braces) for the
 * reads that own rows (whole_read == NULL: the reference's hp_dict) or for every read, "[]" when it owns none (whole_read
 * given: its nonhp_dict, where whole_read[r] != 0 marks the reads to be written in the no-homopolymer form [[[a, b], b]]).
 * keys = the names as JSON string literals back to back, key_bounds their byte offsets.  Returns bytes written (< 0: error;
 * capacity of sum(key bytes) + 48 per row + 40 per read always suffices). */
int64_t cf_chunks_json(const char* keys, const int64_t* key_bounds, int64_t n_reads, const int64_t* bounds,
                       const int64_t* start, const int64_t* end, const uint8_t* whole_read, char* out, int64_t capacity);

/* Ingest on the HOST (no device work, no cf_model): the file read of the reference's per-file loop (catfish/catfish:50-56 ->
 * infer.process_signal, infer.py:77-93) for the read format this image can hold -- one-dimensional C-order little-endian
 * int16 .npy files (DAC codes after the leader trim; there is no HDF5 library here) -- for MANY files at once: a pool of
 * n_threads host threads (<= 0: 4) reads them straight into ONE caller-owned buffer, back to back in the order given.
 * paths: the names as NUL-terminated strings back to back, path_bounds[n_files + 1] their byte offsets; out / capacity: the
 * int16 buffer (e.g. pinned staging memory) and its size in samples; lengths[n_files] receives every read's sample count,
 * *total (may be NULL) their sum (also when they do not fit capacity).  CF_ERR_INVALID names the first file that is
 * missing or is not such an array in cf_last_error(): the caller then takes its general loader for that batch.  A file is
 * judged by its first 4 KiB (its header) and its size before it is read: only regular files whose header matches their
 * length are read whole.  CF_ERR_NOMEM: the tables or a read did not fit host memory (no C++ exception leaves the call). */
int cf_load_npy_int16(const char* paths, const int64_t* path_bounds, int64_t n_files, int16_t* out, int64_t capacity,
                      int64_t* lengths, int64_t* total, int32_t n_threads);

/* Sizes on disk of n_files entries of ONE directory (host code, no device work): the listing step of the reference's per-file
 * loop (catfish/catfish:49-50) -- the sizes cut the sorted file list into blocks of equal work per rank and into batches before
 * anything is read.  names: the entry names (relative to dir) as NUL-terminated strings back to back, name_bounds[n_files + 1]
 * their byte offsets; sizes[n_files] receives st_size (regular files, and whatever else the directory holds: it is judged when
 * its turn to be read comes).  fstatat relative to one directory handle from n_threads host threads (<= 0: 4).  CF_ERR_INVALID
 * names the first entry that cannot be stat-ed (e.g. removed since the listing) in cf_last_error(). */
int cf_stat_files(const char* dir, const char* names, const int64_t* name_bounds, int64_t n_files, int64_t* sizes, int32_t n_threads);

/* The listing of the input directory as an object (host code; catfish/catfish:49-50 `input_files = os.listdir(input_dir)`).  Every
 * rank of a sharded job needs the same ORDER of all names, the sizes of one block of them and the names of the block it ends up
 * classifying -- not a host-language string per entry of a 100 000-file directory on each of 8 ranks.
 *   cf_listing_open   reads all entry names of dir (no "." / ".."), orders them bytewise (= sorted() of the decoded names whenever
 *                     they are valid UTF-8), keeps them; *n_entries their number, digest[2] 128 bits over the ordered names (what
 *                     the ranks compare to make sure they saw the same directory)
 *   cf_listing_sizes  st_size of entries [lo, hi) of that order (fstatat from n_threads host threads, as cf_stat_files)
 *   cf_listing_names  the names of entries [lo, hi), NUL-terminated, back to back into out (capacity bytes) with bounds[hi - lo + 1]
 *                     their offsets; *needed (may be NULL) the bytes they take; out == NULL: size query only
 *   cf_listing_from_names  the same object from names somebody else read and ordered (n_entries NUL-terminated names back to back,
 *                     strictly ascending bytewise -- checked): rank 0 reads the directory ONCE and broadcasts what cf_listing_names
 *                     gave it, because concurrent readdirs of one directory serialise on some file systems (overlayfs: 8 ranks x
 *                     100 000 entries 102 ms each, one reader 13 ms)
 * Not thread-safe per listing; independent listings are. */
typedef struct cf_listing cf_listing;
int cf_listing_open(const char* dir, cf_listing** out, int64_t* n_entries, uint64_t* digest);
int cf_listing_from_names(const char* dir, const char* names, int64_t n_bytes, int64_t n_entries, cf_listing** out, uint64_t* digest);
int cf_listing_sizes(const cf_listing* l, int64_t lo, int64_t hi, int64_t* sizes, int32_t n_threads);
int cf_listing_names(const cf_listing* l, int64_t lo, int64_t hi, char* out, int64_t capacity, int64_t* bounds, int64_t* needed);
void cf_listing_close(cf_listing* l);
/* cf_load_npy_int16 for entries [lo, hi) of a listing, opened relative to the listing's directory: no path string per file is ever
 * built by the caller.  Every entry must be named *.npy; same results, errors and buffers as cf_load_npy_int16. */
int cf_listing_load_npy_int16(const cf_listing* l, int64_t lo, int64_t hi, int16_t* out, int64_t capacity, int64_t* lengths,
                              int64_t* total, int32_t n_threads);

/* The split step, catfish/catfish:85-92 -> split_f5.split_signal (catfish/split_f5.py:8-81), for entries [lo, hi) of a listing that are
 * one-dimensional little-endian int16 .npy reads.  Row r of the two CSR chunk tables (cf_chunks_from_spans' outputs; bounds[hi - lo + 1])
 * belongs to entry lo + r.  Every read WITH homopolymer rows (`for read in hp_dict`, catfish/catfish:88) is read once and cut:
 * signal[start:end] (Python slice rules: a bound below zero counts from the end, both are clamped to the read) of its HP rows goes to
 * <hp_dir>/<stem>_<k>.npy, of its non-HP rows to <nonhp_dir>/<stem>_<k>.npy -- <stem> = the entry's name up to its FIRST dot
 * (split_f5.py:39,65), k = 0, 1, ... over the HP rows and on into the non-HP rows (:34,57,81) -- each file byte for byte numpy.save of that
 * int16 slice.  (The reference writes a gzip-9 HDF5 copy of the input per piece; HDF5 is outside this path.)  Reads sharing a stem overwrite
 * each other's pieces in listing order, as in the reference.  n_threads host threads (<= 0: 4).  counts (may be NULL): int64[4] = reads cut,
 * HP files, non-HP files, samples written.  CF_ERR_INVALID names the first entry that is not such a read (nothing is rolled back: pieces are
 * rewritten whole by whoever repeats the step); CF_ERR_IO names the first file that could not be written, with the system's reason. */
int cf_listing_split_npy_int16(const cf_listing* l, int64_t lo, int64_t hi, const int64_t* hp_bounds, const int64_t* hp_start,
                               const int64_t* hp_end, const int64_t* nonhp_bounds, const int64_t* nonhp_start, const int64_t* nonhp_end,
                               const char* hp_dir, const char* nonhp_dir, int32_t n_threads, int64_t* counts);

/* CRC-32C (Castagnoli) of n bytes, continuing from crc (0 to start): the checksum of leveldb table blocks and of every tensor in a
 * TensorFlow checkpoint-V2 bundle, which the checkpoint reader verifies like tf.train.Saver does (catfish/models/rnn_class.py:191-198). */
uint32_t cf_crc32c(const void* data, int64_t n, uint32_t crc);

/* Training support (BASELINE config 5; the reference's RNN.train_network, catfish/models/rnn_class.py:201-210,
 * differentiates this graph with TensorFlow's autodiff).  One bidirectional GRU layer at a time, fp32 MFMA,
 * on device buffers in the kernels' fragment layout [tile][t][mtile][lane][4] (tile = 16 windows; element
 * (lane, reg) of M-tile m = feature 16m + 4(lane>>4) + reg of window lane&15):
 *   x_frag   [tiles][35][cin/16][64][4]      layer input (cin = 32 for layer 0, 128 above)
 *   y_frag   [tiles][35][8][64][4]           layer output (M-tiles 0-3 forward, 4-7 backward direction)
 *   stash    [tiles][35][2][12][64][4]       activated r, u gates and candidate c of every step
 *   dy_frag  like y_frag                     gradient of the loss w.r.t. the layer output
 *   dy2_frag like y_frag, or NULL            second addend of that gradient (the other direction's dx slab of the
 *                                            layer above, so no separate add pass is needed)
 *   dy_scale like y_frag, or NULL            per-element factor applied to dy (+ dy2): the output-dropout mask
 *                                            divided by keep_prob (DropoutWrapper, rnn_class.py:151-154)
 *   dx_frag  [2][tiles][35][cin/16][64][4]   gradient w.r.t. the layer input, one slab per direction (add them)
 *   da       like stash                      pre-activation gradients da_r, da_u (0-7), da_c (8-11); the weight
 *                                            gradients are dW = A^T dA (cf_gru_train_wgrad)
 * wpack / wpack_bwd: device pointers to the re-tiled weights of BOTH directions ([2][n_floats]), owned by the
 * caller.  cf_gru_pack_map returns the gather map of that re-tiling for one direction, so a trainer can
 * rebuild them on device after every optimizer step: packed[i] = src[idx[i]] * scale[i] with
 * src = [gates_kernel | candidate_kernel | gates_bias | candidate_bias | 0.0] (TF layout, flattened).
 * Call it with idx = scale = NULL to query n_floats. */
int cf_gru_pack_map(int32_t cin, int32_t backward, int32_t* idx, float* scale, int64_t capacity, int64_t* n_floats);
int cf_gru_train_forward(cf_model* m, int32_t cin, const float* wpack, const float* x_frag, float* y_frag,
                         float* stash, int64_t n_windows, void* stream);
int cf_gru_train_backward(cf_model* m, int32_t cin, const float* wpack_bwd, const float* y_frag, const float* stash,
                          const float* dy_frag, const float* dy2_frag, const float* dy_scale, float* dx_frag, float* da,
                          int64_t n_windows, void* stream);
/* One biGRU layer of ANY geometry for training (layer_size a multiple of 16 up to 256; the reference's hyper-parameter search,
 * networks/train_validate.py:66-111, draws 16..256).  These two run the serial part on the any-size kernels (csrc/generic.hpp);
 * everything that is a plain GEMM over all (window, step) pairs -- the input gradient W_x^T da and the weight gradients
 * [x; h]^T da -- is the caller's (catfish_amd/anysize_train.py uses library GEMMs).  Buffers are device pointers, fragment
 * layout, n_windows a multiple of 16:
 *   wpack   [2 dirs][3: r, u, c][H/16][cin_blocks + H/16][64][4]   A fragments, r / u scaled by -log2(e), c by 2 log2(e)
 *   bpack   [2][3][H/16][64][4]                                    biases, same scaling
 *   x_frag  [tiles][35][cin_blocks][64][4]    y_frag [tiles][35][2 H/16][64][4] (forward features first)
 *   stash   [tiles][35][2][3: r, u, c][H/16][64][4]                 activated gates, written by the forward
 *   wtpack  [2 dirs]{ Wc_h^T [H/16][H/16][64][4], Wg_h^T [H/16][2 H/16][64][4] }   unscaled
 *   dy_frag like y_frag (dropout already applied by the caller); da like stash: dL/d(pre-activation) of r, u, c. */
int cf_gru_anysize_train_forward(cf_model* m, int32_t layer_size, int32_t cin_blocks, const float* wpack, const float* bpack,
                                 const float* x_frag, float* y_frag, float* stash, int64_t n_windows, void* stream);
int cf_gru_anysize_train_backward(cf_model* m, int32_t layer_size, const float* wtpack, const float* y_frag, const float* stash,
                                  const float* dy_frag, float* da, int64_t n_windows, void* stream);
/* The launch shape those two calls take for n_windows windows on m's device (csrc/anysize_launch.hpp), without launching anything:
 * out = forward {waves per workgroup, grid x, dynamic LDS bytes, h_via_y}, backward {waves, grid x, LDS bytes, max waves}.  A
 * workgroup runs `waves` tiles of one direction, so grid x * waves >= tiles and the last workgroup may be partly empty.  For
 * tests and tools that must know which regime a size runs in; same argument checks as the two calls. */
int cf_gru_anysize_train_shape(const cf_model* m, int32_t layer_size, int64_t n_windows, int64_t out[8]);
/* The launch shape of the biGRU layers of an any-size model's forward pass (cf_infer* of a geometry other than 64 / 32, or of the
 * plain RNN type in bf16x3) in one pass of n_windows windows, 1 <= n_windows <= the model's windows per pass, without launching
 * anything (csrc/anysize_infer_launch.hpp): out receives one row of five values per biGRU layer, `capacity` >= n_layers rows of
 * room: {kernel: 0 = the LDS-resident kernel of the tuned path (a 64-unit layer with 16 / 32 / 128 inputs in fp32), 1 = one tile
 * per wave, 2 = two tiles per wave; waves per workgroup; grid x; dynamic LDS bytes; h_via_y}.  Waves, grid and LDS are 0 for
 * kernel 0, whose regimes cf_launch_regimes reports.  For tests and tools that must know which launch a size runs in. */
int cf_anysize_infer_shape(const cf_model* m, int64_t n_windows, int64_t* out, int64_t capacity);
/* Training precision "bf16x3" for those two calls: only the matrix products on the serial chain -- forward [x | h] W_g and
 * [x | r.h] W_c, backward Wc_h^T da_c and Wg_h^T [da_r; da_u] -- are evaluated as a_hi w_hi + a_lo w_hi + a_hi w_lo on
 * v_mfma_f32_16x16x32_bf16 (hi = bf16(v), lo = bf16(v - hi)); state, gate activations, stash, da and all accumulation stay fp32,
 * and so does everything GEMM-shaped around them.  Same buffers, launch shapes, argument checks and messages as the fp32 calls,
 * except that the weights come as bf16x3 packs made on the device from the fp32 ones (the weights change every step):
 *   the repack call     one layer's wpack (transposed = 0: rows [2][3][H/16] of K segments [cin_blocks | H/16]) or wtpack
 *                       (transposed = 1: per direction H/16 rows of [H/16], then H/16 rows of [2 H/16]; cin_blocks is ignored) ->
 *                       pack_x3.  Every K segment of k tiles is padded to k' = (k + 3) & ~3; pair p of a segment takes source
 *                       tiles a = 2p, b = 2p + 1 (zeros past k) and writes, per lane, hi = bf16(a[0..3] | b[0..3]) to the
 *                       16-byte slot 2p and lo = bf16(v - hi) to slot 2p + 1 of the padded row (round to nearest even).
 *   the size query      out = {floats of pack_x3 for wpack, for wtpack}: 2 * 3 * H/16 * (cin_blocks' + H/16') * 256 and
 *                       2 * H/16 * (H/16' + (2 H/16)') * 256.
 * bpack is the fp32 call's.  An x3 pack must be rebuilt whenever its fp32 pack changes. */
int cf_gru_anysize_x3_pack_floats(int32_t layer_size, int32_t cin_blocks, int64_t out[2]);
int cf_gen_repack_x3(cf_model* m, int32_t layer_size, int32_t cin_blocks, int32_t transposed, const float* pack, float* pack_x3,
                     void* stream);
int cf_gru_anysize_train_forward_x3(cf_model* m, int32_t layer_size, int32_t cin_blocks, const float* wpack_x3, const float* bpack,
                                    const float* x_frag, float* y_frag, float* stash, int64_t n_windows, void* stream);
int cf_gru_anysize_train_backward_x3(cf_model* m, int32_t layer_size, const float* wtpack_x3, const float* y_frag, const float* stash,
                                     const float* dy_frag, float* da, int64_t n_windows, void* stream);
/* The same two calls with the layer's OUTPUT dropout (DropoutWrapper(output_keep_prob), rnn_class.py:151-154) done inside the
 * kernels, no mask tensor: whether an output element is kept is a hash of (seed, layer, *step_count, element index).  The
 * forward additionally writes y_drop_frag = y * mask / keep_prob (what the next layer or the dense head reads; y_frag itself stays
 * un-dropped for the recurrence and the backward pass); the backward applies the same factor to the incoming gradient when
 * dy_scale is NULL and keep_prob < 1.  step_count: device double[1] (the optimizer's step counter, so every step draws a new mask
 * even under graph replay) or NULL.  cf_dropout_scale writes that factor tensor out (tests / tools only). */
int cf_gru_train_forward_dropout(cf_model* m, int32_t cin, const float* wpack, const float* x_frag, float* y_frag, float* stash,
                                 int64_t n_windows, float* y_drop_frag, float keep_prob, uint32_t seed, int32_t layer,
                                 const double* step_count, void* stream);
int cf_gru_train_backward_dropout(cf_model* m, int32_t cin, const float* wpack_bwd, const float* y_frag, const float* stash,
                                  const float* dy_frag, const float* dy2_frag, const float* dy_scale, float* dx_frag, float* da,
                                  int64_t n_windows, float keep_prob, uint32_t seed, int32_t layer, const double* step_count,
                                  void* stream);
int cf_dropout_scale(cf_model* m, float keep_prob, uint32_t seed, int32_t layer, const double* step_count, int64_t n_windows,
                     float* scale_frag, void* stream);
/* dW of one biGRU layer from the fragment buffers (the weight-gradient half of optimizer.minimize(loss),
 * catfish/models/rnn_class.py:62-71): grads = per direction [ gates kernel [cin+64,128] | gates bias [128] |
 * candidate kernel [cin+64,64] | candidate bias [64] ] in TensorFlow layout, 2 directions back to back.
 * workspace: cf_gru_wgrad_workspace_floats(m, cin, n_windows) floats of device scratch (0 = bad arguments). */
int64_t cf_gru_wgrad_workspace_floats(cf_model* m, int32_t cin, int64_t n_windows);
int cf_gru_train_wgrad(cf_model* m, int32_t cin, const float* x_frag, const float* y_frag, const float* stash, const float* da,
                       int64_t n_windows, float* workspace, int64_t workspace_floats, float* grads, void* stream);

/* Residual conv stack for training (forward catfish/models/resnet_class.py:44-82 with a stash of the conv outputs;
 * backward = its share of optimizer.minimize(loss), rnn_class.py:62-71).  All pointers are device pointers.
 *   params  cf_res_train_param_floats(n_blocks) floats: per conv+BN unit (4 per block, kernel widths 1,1,3,1)
 *           kernel [k][cin][32] | bias[32] | gamma[32] | beta[32] | moving_mean[32] | moving_variance[32], TF layouts,
 *           units back to back; cin = 1 for the first two units, 32 afterwards
 *   x       [n_windows][35] fp32            z_stash [4 n_blocks][n_windows*35][32]     out / d_out [n_windows*35][32]
 *   grads   same offsets as params (kernel, bias, gamma, beta gradients; the moving statistics get 0)
 *   workspace  cf_res_train_workspace_floats(n_blocks, n_windows) floats of scratch (per-workgroup partial sums,
 *           added in a fixed order) */
int64_t cf_res_train_param_floats(int32_t n_blocks);
int64_t cf_res_train_workspace_floats(int32_t n_blocks, int64_t n_windows);
int cf_res_train_forward(cf_model* m, int32_t n_blocks, const float* params, const float* x, float* z_stash, float* out,
                         int64_t n_windows, void* stream);
int cf_res_train_backward(cf_model* m, int32_t n_blocks, const float* params, const float* x, const float* z_stash,
                          const float* d_out, float* workspace, int64_t workspace_floats, float* grads, int64_t n_windows,
                          void* stream);

/* Dense head + loss of the training step, forward and backward in one pass (RNN.output_layer + RNN.compute_loss,
 * catfish/models/rnn_class.py:178-183,74-79: final_fully_connected followed by tf.losses.sigmoid_cross_entropy, mean over
 * all n_windows * 35 elements).  y_frag: the dense layer's input = last biGRU layer's output after output dropout, fragment
 * layout [tiles][35][8][64][4]; labels: device fp32 [n_windows][35]; dense_kernel [128], dense_bias [1]: device pointers.
 * Writes dy_frag (d loss / d y_frag, same layout), grads = d kernel [128] | d bias [1], loss[0] = the mean loss, and the
 * logits [n_windows][35] when that pointer is not NULL.  workspace: cf_train_head_workspace_floats(m, n_windows) floats. */
int64_t cf_train_head_workspace_floats(cf_model* m, int64_t n_windows);
int cf_train_head(cf_model* m, const float* y_frag, const float* dense_kernel, const float* dense_bias, const float* labels,
                  int64_t n_windows, float* dy_frag, float* logits, float* workspace, int64_t workspace_floats, float* grads,
                  float* loss, void* stream);

/* One optimizer step over ALL variables at once (optimizer.minimize(loss), rnn_class.py:62-71): params, grads and the two slot
 * variables are flat device buffers of one layout, n floats each.  kind 0 = tf.train.RMSPropOptimizer(lr) (decay 0.9,
 * momentum 0, epsilon 1e-10; slot1 = rms, initial value 1; slot2 = momentum), kind 1 = tf.train.AdamOptimizer(lr) (beta 0.9 /
 * 0.999, epsilon 1e-8; slot1 = m, slot2 = v).  step_count: device double[1], steps taken so far; read by the update (Adam's bias
 * correction) and incremented by this call.  When n_packed > 0 the updated weights are re-tiled for the biGRU kernels in the
 * same call: packed[i] = params[pack_idx[i]] * pack_scale[i] (indices from cf_gru_pack_map, rebased into params). */
int cf_opt_step(cf_model* m, int32_t kind, float* params, const float* grads, float* slot1, float* slot2, int64_t n, float lr,
                double* step_count, const int32_t* pack_idx, const float* pack_scale, float* packed, int64_t n_packed, void* stream);

/* Whole-step training of ANY geometry (csrc/gen_train.hpp; catfish_amd/anysize_step.py drives it): the pieces around
 * cf_gru_anysize_train_forward / _backward, so that conv stack, dropout, dense head, loss, backward and optimizer all run on these
 * kernels.  fp32, run-time sizes, device pointers, every launch on `stream` with no host synchronisation (graph-capturable).
 * n_windows: a positive multiple of 16 (padding windows hold zeros; their gradients arrive as exact zeros).  Every activation is a
 * fragment plane [tiles][35][F/16][64][4] (F features; element (window n, step t, feature f) at
 * ((((n / 16) * 35 + t) * F/16 + f / 16) * 64 + 16 ((f / 4) % 4) + n % 16) * 4 + f % 4), except a single input feature (cin = 1),
 * which is [n_windows][35].  Channel counts (cin, cout, features) are multiples of 16 up to 512 unless stated.
 *   unit         one conv + BN unit in TF layout: kernel [kw][cin][cout] | bias | gamma | beta | moving_mean | moving_variance;
 *                unit_grads has the same layout (the moving statistics are not written)
 *   layer_params one biGRU layer, per direction (fw, bw): gates kernel [cin + H][2H] | gates bias [2H] | candidate kernel [cin + H][H]
 *                | candidate bias [H]; layer_grads the same
 *   dense        final_fully_connected kernel [features] | bias [1]; dense_grads the same
 * Gradients are sums over all positions, produced as per-workgroup partials over fixed chunks of 32 windows and reduced in chunk
 * order (no atomics): the same inputs give bit-identical gradients.  Workspaces: cf_gen_train_workspace_floats(rows, cols,
 * n_windows) for a weight gradient of rows x cols (conv: kw cin + 1 rows x cout; GRU: cin + H + 1 rows x 2H), n_windows / 16 x 2
 * cout for cf_gen_bn_backward, cf_gen_head_workspace_floats for the head.  A bad size, a null buffer or a short workspace is
 * CF_ERR_INVALID.
 *   cf_gen_conv_forward        z_stash = conv(x) + bias (SAME padding inside each window, kw 1 or 3), out = [ReLU](z s + t) with
 *                              s = gamma / sqrt(var + 1e-3), t = beta - mean s; with shortcut: out = ReLU(out + shortcut)
 *   cf_gen_bn_backward         dz = g [mask > 0] [z s + t > 0 if relu] s (mask optional: the block output after the shortcut's
 *                              ReLU); d gamma, d beta into unit_grads
 *   cf_gen_conv_wgrad          d kernel, d bias of the unit (x is the unit's input) into unit_grads
 *   cf_gen_conv_backward_data  dx = conv^T(dz) (+ add)
 *   cf_gen_gru_dx              dx = sum over directions and gates of da W_x^T (da as written by cf_gru_anysize_train_backward)
 *   cf_gen_gru_wgrad           [x; h_prev]^T da_{r,u}, [x; r h_prev]^T da_c and the bias sums of both directions into layer_grads
 *                              (x_frag with ceil(cin / 16) feature tiles, y_frag the layer's output before dropout)
 *   cf_gen_dropout             out = in * mask / keep_prob over a [tiles][35][2H/16][64][4] plane: the mask is the tuned kernels'
 *                              hash of (seed, layer, *step_count, f32x4 index) (the same masks as cf_gru_train_forward_dropout at
 *                              H = 64), or out = in * scale_frag when scale_frag is not NULL.  Also the backward of the dropout.
 *   cf_gen_head                logits, mean sigmoid cross-entropy over the n_real real windows (loss[0]), d input, d dense;
 *                              logits [n_windows][35] or NULL; labels [n_windows][35]; n_real in (n_windows - 16, n_windows]
 *   cf_gen_x_frag              the one input feature [n_windows][35] as a 16-feature plane (zeros above feature 0) */
int64_t cf_gen_train_workspace_floats(int32_t rows, int32_t cols, int64_t n_windows);
int64_t cf_gen_head_workspace_floats(int32_t features, int64_t n_windows);
int cf_gen_conv_forward(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* unit, const float* x, const float* shortcut,
                        int32_t relu, float* z_stash, float* out, int64_t n_windows, void* stream);
int cf_gen_conv_backward_data(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* unit, const float* dz, const float* add,
                              float* dx, int64_t n_windows, void* stream);
int cf_gen_bn_backward(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* unit, const float* g, const float* mask,
                       int32_t relu, const float* z_stash, float* dz, float* workspace, int64_t workspace_floats, float* unit_grads,
                       int64_t n_windows, void* stream);
int cf_gen_conv_wgrad(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* x, const float* dz, float* workspace,
                      int64_t workspace_floats, float* unit_grads, int64_t n_windows, void* stream);
int cf_gen_gru_dx(cf_model* m, int32_t layer_size, int32_t cin, const float* layer_params, const float* da, float* dx, int64_t n_windows,
                  void* stream);
int cf_gen_gru_wgrad(cf_model* m, int32_t layer_size, int32_t cin, const float* x_frag, const float* y_frag, const float* stash,
                     const float* da, float* workspace, int64_t workspace_floats, float* layer_grads, int64_t n_windows, void* stream);
int cf_gen_dropout(cf_model* m, int32_t layer_size, float keep_prob, uint32_t seed, int32_t layer, const double* step_count,
                   const float* scale_frag, const float* in_frag, float* out_frag, int64_t n_windows, void* stream);
int cf_gen_head(cf_model* m, int32_t features, const float* in_frag, const float* dense, const float* labels, int64_t n_real,
                float* din_frag, float* logits, float* workspace, int64_t workspace_floats, float* dense_grads, float* loss,
                int64_t n_windows, void* stream);
int cf_gen_x_frag(cf_model* m, const float* x, float* x_frag, int64_t n_windows, void* stream);

/* Backward of the inference function (csrc/gen_train.hpp; catfish_amd/op_grad.py drives it for the autograd formula of
 * torch.ops.catfish.resnetrnn_forward): inference-mode BN on the moving statistics, no dropout, p = sigmoid(logit).  The
 * forward and the rest of the backward are the cf_gen_* calls above; conventions (fragment planes, unit / layer_params / dense
 * layouts, n_windows, fixed-order reductions, stream, CF_ERR_INVALID on a bad size, a null buffer or a short workspace) as there.
 *   cf_gen_head_backward       from the last layer's output plane in_frag [.., features], the dense weights and an upstream
 *                              dprobs [n_windows][35]: dlogit = g sigmoid(z) sigmoid(-z) (stable for any z), din_frag = dlogit w;
 *                              d dense into dense_grads unless it is NULL (then no reduction is launched).  Workspace:
 *                              cf_gen_head_backward_workspace_floats(features, n_windows)
 *   cf_gen_signal_grad         dx [n_windows][35], d loss / d the one input feature, one fixed summation order per position.
 *                              ResNetRNN: layer_size 0, channels C; params0 / grad0 the shortcut unit (conv1d, kw 1, cin 1) and
 *                              its dz, params1 / grad1 the first conv unit (conv1d_1) and its dz (cf_gen_bn_backward's output):
 *                              dx = sum_o dz_sc[o] w_sc[o] + dz_1[o] w_1[o].  Plain RNN: channels 0, layer_size H; params0 layer
 *                              0's layer_params (cin 1), grad0 its da; params1, grad1 NULL
 *   cf_gen_bn_backward_data    dz of cf_gen_bn_backward without d gamma, d beta (no workspace, no reduction)
 *   cf_gen_bn_stat_grads       the moving-statistics slots of unit_grads from its d gamma, d beta (written by
 *                              cf_gen_bn_backward): d mean = -gamma d beta / sqrt(var + 1e-3), d var = -gamma d gamma / (2 (var + 1e-3)) */
int64_t cf_gen_head_backward_workspace_floats(int32_t features, int64_t n_windows);
int cf_gen_head_backward(cf_model* m, int32_t features, const float* in_frag, const float* dense, const float* dprobs, float* din_frag,
                         float* workspace, int64_t workspace_floats, float* dense_grads, int64_t n_windows, void* stream);
int cf_gen_signal_grad(cf_model* m, int32_t layer_size, int32_t channels, const float* params0, const float* grad0, const float* params1,
                       const float* grad1, float* dx, int64_t n_windows, void* stream);
int cf_gen_bn_backward_data(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* unit, const float* g, const float* mask,
                            int32_t relu, const float* z_stash, float* dz, int64_t n_windows, void* stream);
int cf_gen_bn_stat_grads(cf_model* m, int32_t kw, int32_t cin, int32_t cout, const float* unit, float* unit_grads, void* stream);

/* Device-resident training set (csrc/sample_batch.hpp; catfish_amd/device_db.py states the sampler on the host and
 * DeviceExampleDb.batch_indices is its definition): the next balanced batch of the reference's sampler (ExampleDb.get_training_set,
 * networks/trainingDB/ExampleDb.py:57-83: size / ratio distinct positives, the rest distinct negatives, shuffled, uniform labels)
 * drawn and gathered on the card, so that a captured training step feeds itself.
 *   pos [n_pos][35], neg [n_neg][35]   the two pools of windows, device float32
 *   draw_counter                       device int64[1]: the number of this draw.  Read by every workgroup (a replayed graph draws a
 *                                      new batch each time) and incremented by a one-thread launch of this call after them
 *   x [size][35], y [>= size][35]      the step's input and label buffers; rows of y past size are not touched
 * Every slot evaluates three keyed bijections (a four-round Feistel network over the next even-bit power of two, round function
 * the murmur3 finaliser, cycle-walking) of (seed, draw): slot -> rank over [0, size), rank -> pool row over [0, n_pos) for ranks
 * below size / ratio and over [0, n_neg) for the others.  No state, no atomics.  m may be NULL (the current device is used).
 * CF_ERR_INVALID when a pool is smaller than its share.
 * cf_sample_batch_logged: the same, and its one-thread launch also keeps the losses of a chain of replayed steps on the card:
 * with p = *log_pos (device int64[1]) it stores prev_loss[0] -- the loss of the step before this draw, still in the step's loss
 * buffer -- to log[p - 1] when 1 <= p <= capacity, then *log_pos = p + 1.  The chain's last loss is read from prev_loss itself. */
int cf_sample_batch(cf_model* m, const float* pos, int64_t n_pos, const float* neg, int64_t n_neg, int64_t size, int32_t ratio,
                    uint32_t seed, int64_t* draw_counter, float* x, float* y, void* stream);
int cf_sample_batch_logged(cf_model* m, const float* pos, int64_t n_pos, const float* neg, int64_t n_neg, int64_t size, int32_t ratio,
                           uint32_t seed, int64_t* draw_counter, float* x, float* y, const float* prev_loss, float* log, int64_t capacity,
                           int64_t* log_pos, void* stream);

/* Device-resident validation set (csrc/validation.hpp; catfish_amd/device_validation.py states both steps in numpy --
 * DeviceValidationSet.pack and score_host are their definitions): one checkpoint round (networks/train_validate.py:188-295) packed and
 * scored on the card.  Both calls are asynchronous on `stream` and capturable; m may be NULL (the current device is used).
 *   signal [signal_total] float32, labels [signal_total] uint8     all reads concatenated, device
 *   src_first [n], length [n], bounds [n + 1]                      device int64: read r's stretch starts at signal[src_first[r]], has
 *                                                                  length[r] samples and fills packed samples bounds[r] .. bounds[r + 1]
 *   total = bounds[n]; longest = the largest bounds[r + 1] - bounds[r] (sizes the grid only: any value <= total gives the same result)
 * cf_validation_gather: x_out / y_out [total]; packed sample bounds[r] + i is signal / labels [src_first[r] + i] for i < length[r] and
 * 0 / 0 after it (the zero tail up to the window multiple).  A table entry that points outside signal or x_out moves nothing.
 * cf_validation_score: with p, z the probability and the logit of a sample as doubles and y its label value,
 *   right_out[r]  (int64)   samples of read r with rint(p) == y (half to even: p = 0.5 rounds to 0)
 *   ce_sum_out[r] (double)  sum over read r of max(z, 0) - z y + log1p(exp(-|z|))
 *   counts_out[4 k ..]      (int64) over ALL samples, called = p >= thresholds[k] (device double [n_thresholds], 1..16 of them):
 *                           called & y == 1, called & y != 1, !called & y == 0 (zero tails included), !called & y != 0
 * A read is cut into chunks of cf_validation_score_chunk() samples, one workgroup each, reduced in a fixed order into a slot of
 * `partials` (device double [partial_slots], partial_slots >= total / chunk + n); a second launch adds a read's slots in chunk order.
 * No floating-point atomics: equal inputs give equal bits.  CF_ERR_INVALID for n < 1, n_thresholds outside 1..16 or too few slots. */
int cf_validation_score_chunk(void);
int cf_validation_gather(cf_model* m, const float* signal, const uint8_t* labels, int64_t signal_total, const int64_t* src_first,
                         const int64_t* length, const int64_t* bounds, int64_t n, int64_t total, int64_t longest, float* x_out,
                         uint8_t* y_out, void* stream);
int cf_validation_score(cf_model* m, const float* probs, const float* logits, const uint8_t* y, const int64_t* bounds, int64_t n,
                        int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds, int64_t* right_out,
                        double* ce_sum_out, int64_t* counts_out, double* partials, int64_t partial_slots, void* stream);

/* Event-level validation (csrc/validation_runs.hpp; device_validation.run_states_host is its definition): the reference's offline
 * networks/process_output.py:235-273 on the card.  Stretch r is the first length[r] packed samples from bounds[r] (its zero tail is not
 * part of it).  Per threshold t: pred = correct_short((double)p >= t, min_run) inside every stretch; a run is a maximal run of ones,
 * and -- hp_loc_dict's rule (:633-636) -- a run whose last one sits at n - 2 ends at n - 1.  Kind 0 = the runs of y == 1 judged against
 * pred, kind 1 = the runs of pred judged against y; state 0 = complete (the other array is 1 over the whole run), 2 = absent (0 over
 * the whole run), 1 = incomplete; a run of L samples falls into bin #{j : edges[j] <= L}.
 *   counts_out   device int64 [n_thresholds][2][n_edges + 1][3], zeroed and written by the call
 *   thresholds   HOST double [n_thresholds], 1..16 of them;  edges  HOST int64 [n_edges], 0..7, positive and strictly ascending
 *   work         device bytes, >= cf_validation_run_work_bytes(total, n_thresholds) (one corrected-label array per threshold);
 *                16-byte aligned for the bit-mask post-processing kernel, otherwise the per-sample one runs
 * A workgroup walks a stretch in pieces of cf_validation_run_piece() samples and counts a run once, where it ends; integer
 * arithmetic only, so equal inputs give equal results whatever `longest` (a hint, as above) or the grid.  Asynchronous on `stream`;
 * m may be NULL.  CF_ERR_INVALID before any launch for a null pointer, n outside [1, 2^31), total >= 2^31, n_thresholds outside 1..16,
 * more than 7 edges, edges not positive and ascending, min_run < 1 or too small a work buffer. */
int cf_validation_run_piece(void);
int64_t cf_validation_run_work_bytes(int64_t total, int32_t n_thresholds);
int cf_validation_run_states(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length, int64_t n,
                             int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds, const int64_t* edges,
                             int32_t n_edges, int32_t min_run, int64_t* counts_out, void* work, int64_t work_bytes, void* stream);

/* ... with pred = correct_short(bridge_gaps((double)p >= t, max_gap), min_run) inside every stretch (cf_postprocess_spans_bridged's
 * rule and domain: max_gap == 0 is cf_validation_run_states; otherwise min_run + max_gap <= 64 and a 16-byte aligned work buffer, else
 * CF_ERR_INVALID before any launch).  The work size is the same. */
int cf_validation_run_states_bridged(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length,
                                     int64_t n, int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds,
                                     const int64_t* edges, int32_t n_edges, int32_t max_gap, int32_t min_run, int64_t* counts_out,
                                     void* work, int64_t work_bytes, void* stream);

/* Border-level validation (csrc/validation_borders.hpp, csrc/validation_borders_word.hpp; device_validation.run_borders_host is its
 * definition): the rest of what the reference's check_hp (networks/process_output.py:814-895) returns for a run.  Stretches,
 * prediction, runs and kinds as for cf_validation_run_states; a label other than 1 counts as 0.  For every run [s, e] that is not
 * absent, with o the other array: l = -(ones of o right before s, position 0 never counted) when o[s] == 1, else the zeros of o from s
 * to its first one; r = the ones of o right after e when o[e] == 1, else -(the zeros of o from e down to its last one); an
 * interruption is a maximal run of zeros of o inside [s, e] that touches neither end.  With R = reach a (threshold, kind) row is
 * 5 R + 3 cells: [0, 2R+1) histogram of clip(l, -R, R) + R; [2R+1, 4R+2) of clip(r, -R, R) + R; [4R+2, 5R+2) of min(g, R) - 1 over
 * the interruption lengths g; [5R+2] runs with at least one interruption.
 *   counts_out   device int64 [n_thresholds][2][5 * reach + 3], zeroed and written by the call
 *   thresholds   HOST double [n_thresholds], 1..16 of them;  reach  1 .. 128
 *   work         device bytes, >= cf_validation_run_borders_work_bytes(total, n_thresholds) (= cf_validation_run_work_bytes: the two
 *                calls can share one buffer); 16-byte aligned for the bit-mask post-processing kernel
 * A workgroup walks a stretch twice, forward and mirrored, in pieces of cf_validation_run_piece() samples; integer arithmetic only,
 * so equal inputs give equal results whatever `longest` (a hint) or the grid.  Asynchronous on `stream`; m may be NULL.
 * CF_ERR_INVALID before any launch for a null pointer, n outside [1, 2^31), total >= 2^31, n_thresholds outside 1..16, reach outside
 * 1..128, min_run < 1 or too small a work buffer. */
int64_t cf_validation_run_borders_work_bytes(int64_t total, int32_t n_thresholds);
int cf_validation_run_borders(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length, int64_t n,
                              int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds, int32_t reach,
                              int32_t min_run, int64_t* counts_out, void* work, int64_t work_bytes, void* stream);

/* ... with the bridged prediction of cf_validation_run_states_bridged (same rule, same domain, same work size). */
int cf_validation_run_borders_bridged(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length,
                                      int64_t n, int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds,
                                      int32_t reach, int32_t max_gap, int32_t min_run, int64_t* counts_out, void* work,
                                      int64_t work_bytes, void* stream);

/* Validation by base (csrc/validation_bases.hpp, csrc/validation_bases_word.hpp; device_validation.run_bases_host is its definition):
 * the runs of cf_validation_run_states -- same stretches, prediction, runs, kinds and states -- counted by the bases they hold instead of
 * by their length in samples (the reference's prediction_information / get_bases, networks/process_output.py).  basemap is the set's
 * base map as cf_label_events writes it (the event's base byte, bit 7 on the event's centre sample), read in place: the base map of
 * packed sample bounds[r] + i is basemap[src_first[r] + i] (an index outside [0, basemap_total) counts as no base).  The bases of a run are
 * the marked samples inside it (the sample the last-sample rule adds included); nb = how many.  Class 0..3 = A / C / G / T: nb >= 1 and every
 * one of them is that upper-case byte; class 4 = anything else, nb == 0 included.  Bin = min(nb, max_bases).
 *   counts_out   device int64 [n_thresholds][2][3][5][max_bases + 1] (kind, state, class, bin), zeroed and written by the call
 *   thresholds   HOST double [n_thresholds], 1..16 of them;  max_bases  1 .. 32;  src_first  device int64 [n]
 *   work         device bytes, >= cf_validation_run_work_bytes(total, n_thresholds); max_gap as for cf_validation_run_states_bridged
 * Integer arithmetic only, so equal inputs give equal results whatever `longest` (a hint) or the grid.  Asynchronous on `stream`; m may
 * be NULL.  CF_ERR_INVALID before any launch for what cf_validation_run_states_bridged refuses, a null base map or src_first,
 * basemap_total outside [1, 2^31) or max_bases outside 1..32. */
int cf_validation_run_bases(cf_model* m, const float* probs, const uint8_t* y, const uint8_t* basemap, int64_t basemap_total,
                            const int64_t* src_first, const int64_t* bounds, const int64_t* length, int64_t n, int64_t total,
                            int64_t longest, const double* thresholds, int32_t n_thresholds, int32_t max_bases, int32_t max_gap,
                            int32_t min_run, int64_t* counts_out, void* work, int64_t work_bytes, void* stream);

/* Validation curves (csrc/validation_curve.hpp; device_validation.curve_host is its definition): the histogram of a round's
 * probabilities from which the host draws the whole ROC and precision-recall curves (device_validation.curves_from_histogram).
 * With NB = (0x3F800000 >> shift) + 1 bins, a probability with float32 bits u falls into bin min(max((int32_t)u, 0) >> shift, NB - 1)
 * (csrc/validation_curve_bin.hpp), so for p in [0, 1]: p >= the float with bits b << shift  <=>  bin(p) >= b.
 *   hist_out     device int64 [3][NB] (rows: label == 1, label == 0, any other label), zeroed and written by the call; only the
 *                first length[r] samples from bounds[r] of every stretch are counted (the zero tails are not)
 *   shift        10 .. 22 (14: NB = 65 025);  hist_capacity  entries of hist_out, >= 3 NB
 * One workgroup per cf_validation_score_chunk() samples sorts its cells in LDS and issues one 64-bit integer atomic per DISTINCT
 * cell; integers only, so equal inputs give equal results whatever `longest` (a hint, as above).  Asynchronous on `stream`; m may be
 * NULL.  CF_ERR_INVALID before anything is written for a null pointer, n outside [1, 2^31), a shift outside 10 .. 22, a bad size or
 * hist_capacity < 3 NB. */
int cf_validation_curve(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length, int64_t n,
                        int64_t total, int64_t longest, int32_t shift, int64_t* hist_out, int64_t hist_capacity, void* stream);

/* Scores under runs (csrc/validation_scores.hpp, csrc/validation_scores_word.hpp; device_validation.run_scores_host is its
 * definition): the probabilities of the samples under the runs of every state -- what the reference's offline check_for_false_neg
 * (networks/process_output.py:15-137) collects for the missed homopolymers.  Stretches, prediction (bridged when max_gap > 0, under
 * cf_validation_run_states_bridged's domain rule), runs, kinds and states as for cf_validation_run_states.  With NB the bins of
 * cf_validation_curve at `shift`, every sample of a run of kind q and state s at threshold k adds one to cell bin(p) of row
 * [k][q][s] and floor(p * 2^32) (NaN and p < 0 as 0, p > 1 as 2^32) to the row's last cell.
 *   table_out    device int64 [n_thresholds][2][3][NB + 1], zeroed and written by the call;  table_capacity  its entries
 *   thresholds   HOST double [n_thresholds], 1..16 of them;  shift  14 .. 22 (16: NB = 16 257)
 *   work         device bytes, >= cf_validation_run_scores_work_bytes(total, n_thresholds) (twice cf_validation_run_work_bytes: the
 *                labels and, behind them, one byte of paint per sample); 16-byte aligned for the bit-mask post-processing kernel
 * Two launches behind the label passes: a workgroup walks a stretch mirrored and forward and paints every sample with the state of
 * its run, then one workgroup per cf_validation_score_chunk() samples sorts its cells in LDS and issues one 64-bit integer atomic per
 * DISTINCT cell and one per non-zero sum.  Integers only, so equal inputs give equal results whatever `longest` (a hint) or the grid.
 * Asynchronous on `stream`; m may be NULL.  CF_ERR_INVALID before any launch for a null pointer, n outside [1, 2^31), total >= 2^31,
 * n_thresholds outside 1..16, a shift outside 14 .. 22, min_run < 1, a (min_run, max_gap) pair outside the bridging domain,
 * table_capacity or work_bytes too small (the message names the size needed). */
int64_t cf_validation_run_scores_work_bytes(int64_t total, int32_t n_thresholds);
int cf_validation_run_scores(cf_model* m, const float* probs, const uint8_t* y, const int64_t* bounds, const int64_t* length, int64_t n,
                             int64_t total, int64_t longest, const double* thresholds, int32_t n_thresholds, int32_t shift, int32_t max_gap,
                             int32_t min_run, int64_t* table_out, int64_t table_capacity, void* work, int64_t work_bytes, void* stream);

/* Shifted-window voting (csrc/tilings.hpp, index rules in csrc/tilings_rule.hpp; catfish_amd/tilings.py states both steps in numpy --
 * retile_host and vote_host are their definitions).  A read is cut into 35-sample windows at one fixed phase; these two calls let the
 * same reads go through the forward pass in K tilings whose window borders fall phi_j samples apart, and merge the per-sample
 * results.  Base layout: offsets [n_reads + 1] / lengths [n_reads], device int64 -- read r owns packed samples offsets[r] ..
 * offsets[r + 1] (multiples of 35), the first lengths[r] real, total = offsets[n_reads].  One buffer of
 *   tiling size = total + (K - 1) * (total + 35 n_reads)
 * samples holds the base region [0, total) and behind it tiling j >= 1 at T_j = total + (j - 1) * (total + 35 n_reads); read r of
 * tiling j starts at T_j + offsets[r] + 35 r and is one window longer than in the base layout.
 *   phases   HOST int32 [n_phases]: 1..8 strictly ascending ints in 0 .. 34, the first one 0; they travel by value in the kernel
 *            arguments, so nothing is copied and both calls are asynchronous on `stream` and capturable.  m may be NULL (the
 *            current device is used).
 * cf_retile_windows: x[T_j + offsets[r] + 35 r + phi_j + i] = x[offsets[r] + i] for i < lengths[r], and every other sample of the
 * tiling regions 0 -- one launch writes all K - 1 regions completely.  n_phases == 1 launches nothing.
 * cf_vote_tilings: for i < lengths[r], with t_j = (i + phi_j) % 35, p_0 = probs[offsets[r] + i] and p_j the same sample in tiling j,
 *   probs_out[offsets[r] + i] = float32((sum_j w(t_j) * double(p_j)) / (sum_j w(t_j))),  both sums in double in the order j = 0 .. K - 1,
 * with w(t) = 1 (weight 0, "mean") or min(t + 1, 35 - t) (weight 1, "centre").  Samples of the zero tails keep the base value.
 * logits (NULL ok; logits_out NULL exactly then) are merged by the same formula on their own values: the voted logit is the weighted
 * mean of the logits, not the logit of the voted probability.  probs_out [total] may be probs itself (logits_out, logits).
 * n_phases == 1 launches nothing, except that the outputs are copied when they are other buffers.
 * A table entry that is not what the layout promises -- a length that is negative or longer than its region, an offset outside
 * 0 .. total or not a multiple of 35, a descending pair of offsets -- makes that read's tiling regions zero and its vote the base
 * value; where offsets descend, the reads beside the pair may come out so as well.  Whatever the tables hold, nothing is read or
 * written outside [0, tiling size) of x / probs / logits and [0, total) of the outputs.
 * CF_ERR_INVALID before any launch for a null pointer, a negative size, more than 2^31 - 1 reads or 2^40 samples, total % 35 != 0,
 * phases that break the rule above, or an unknown weight. */
int cf_retile_windows(cf_model* m, float* x, const int64_t* offsets, const int64_t* lengths, int64_t n_reads, int64_t total,
                      const int32_t* phases, int32_t n_phases, void* stream);
int cf_vote_tilings(cf_model* m, const float* probs, const float* logits, const int64_t* offsets, const int64_t* lengths,
                    int64_t n_reads, int64_t total, const int32_t* phases, int32_t n_phases, int32_t weight, float* probs_out,
                    float* logits_out, void* stream);

/* Labels from event tables (csrc/label_events.hpp, index rules in csrc/label_events_rule.hpp; catfish_amd/labelling.py states the
 * result in numpy -- event_classes_host, expand_events_host and base_map_host are the definitions).  A batch of resquiggled reads,
 * packed, all device memory: read r owns events event_offsets[r] .. event_offsets[r + 1] (int64 [n_reads + 1]) of bases (uint8
 * [n_events], the base byte, below 128) and lengths (int32 [n_events], samples, >= 1), clipped[2 r] / clipped[2 r + 1] (int32) are
 * its clipped_start / clipped_end, and it owns samples sample_offsets[r] .. sample_offsets[r + 1] (int64 [n_reads + 1], the sum of
 * its lengths apart) of the outputs; total = sample_offsets[n_reads].  With oh = kmer / 2 and E the read's events:
 *   core[e]  = clipped_start <= e < E - clipped_end, e - oh >= 0, e + oh < E, and events e - oh .. e + oh are one byte that is not 'N'
 *   cls[e]   = some core within two events of e (inside the read; the widening ignores clipping and 'N')
 *   labels_out[first sample of e .. + length)  = cls[e]
 *   basemap_out (NULL ok) there = the base byte, bit 7 set on the one sample first + length / 2
 * work: device scratch of the work-bytes query below for n_events (the events' first samples, int32, and classes), 4-byte aligned.
 * Two launches, asynchronous on `stream`, capturable; integers only and no atomics, so equal inputs give equal bytes.  m may be NULL
 * (the current device is used).  The tables are not trusted: a length < 1 contributes nothing, a read whose event range leaves
 * [0, n_events] has no events, samples that no event covers get label 0 and base 0, a read whose sample range leaves [0, total] is
 * not written, and whatever the tables hold nothing is read or written outside the buffers.
 * CF_ERR_INVALID before any launch for a null pointer, a negative size, 2^31 or more events or samples, an even kmer or one outside
 * 1 .. 15, more than 2^23 workgroups (n_reads + total / 4096) or a work buffer that is too small; total == 0 is CF_OK with nothing
 * launched. */
int64_t cf_label_events_work_bytes(int64_t n_events);
int cf_label_events(cf_model* m, const uint8_t* bases, const int32_t* lengths, const int64_t* event_offsets, const int32_t* clipped,
                    const int64_t* sample_offsets, int64_t n_reads, int64_t n_events, int64_t total, int32_t kmer, uint8_t* labels_out,
                    uint8_t* basemap_out, void* work, int64_t work_bytes, void* stream);

/* Labels from a basecaller's move table (csrc/label_moves.hpp, index and arithmetic rules in csrc/label_moves_rule.hpp;
 * catfish_amd/labelling.py states the result in numpy -- merge_moves_host, move_classes_host and MoveBatch.label_host are the
 * definitions).  The reads have NOT been resquiggled: the table is the basecaller's own.  A batch, packed, all device memory: read r
 * owns events event_offsets[r] .. event_offsets[r + 1] of states (uint8 [n_events][k], the model_state k-mer, bytes below 128),
 * lengths (float [n_events], or double with lengths_f64 = 1: SECONDS, finite and > 0) and moves (int32 [n_events]);
 * clipped[2 r] / clipped[2 r + 1] are its clipped_start / clipped_end counted in merged events, n_raw[r] (int64) the samples of its
 * raw signal, and it owns samples sample_offsets[r] .. sample_offsets[r + 1] of the outputs (its `final` apart, below); total =
 * sample_offsets[n_reads].  An event with move != 0 -- and the read's first event whatever its move -- is a head; a head and the
 * events with move == 0 behind it are one merged event.  With M merged events in the read:
 *   n[j]     = ceil(L * 4000), L = the lengths of merged event j summed left to right from its head in the table's own type (for
 *              j = 0 the first length counts twice, as the reference's loop has it), the product in that type too
 *   final    = min(n[0] + .. + n[M - 1], n_raw): the labels the read yields (the caller sizes sample_offsets from it)
 *   core[j]  = clipped_start <= j < M - clipped_end and the head's k bytes are one byte that is not 'N'
 *   cls[j]   = some core within two merged events of j, inside the read
 *   labels_out[first sample of j .. + n[j]), below final  = cls[j]
 *   basemap_out (NULL ok) there = the k-mer's byte k / 2, bit 7 set on the one sample first + n[j] / 2
 * work: device scratch of the work-bytes query below, 4-byte aligned: the merged events compacted per read, then M and final per read
 * as int32 [n_reads][2] at byte 8 * n_events.  Three launches (merge, classes, and cf_label_events' own expansion), asynchronous on
 * `stream`, capturable; no atomics, sums in a fixed order, so equal inputs give equal bytes.  m may be NULL (the current device is
 * used).  The tables are not trusted: a sum whose product with 4000 is not a finite number > 0 contributes no samples, counts and
 * running sums saturate at 2^31 - 1, a read whose event range leaves [0, n_events] has no events, samples that no merged event covers
 * get label 0 and base 0, a read whose sample range leaves [0, total] is not written, and whatever the tables hold nothing is read
 * or written outside the buffers.
 * CF_ERR_INVALID before any launch for a null pointer, a negative size, 2^31 or more events or samples, k outside 1 .. 15,
 * lengths_f64 other than 0 or 1, misaligned lengths, more than 2^23 workgroups (n_reads + total / 4096) or a work buffer that is too
 * small; total == 0 is CF_OK with nothing launched. */
int64_t cf_label_moves_work_bytes(int64_t n_reads, int64_t n_events);
int cf_label_moves(cf_model* m, const uint8_t* states, const void* lengths, int32_t lengths_f64, const int32_t* moves,
                   const int64_t* event_offsets, const int32_t* clipped, const int64_t* n_raw, const int64_t* sample_offsets,
                   int64_t n_reads, int64_t n_events, int64_t total, int32_t k, uint8_t* labels_out, uint8_t* basemap_out, void* work,
                   int64_t work_bytes, void* stream);

/* Per-base calls (csrc/base_votes.hpp, index and arithmetic rules in csrc/base_votes_rule.hpp; catfish_amd/base_votes.py states the
 * result in numpy -- vote_host is the definition).  The samples of every base of a round's stretches vote on it, and the voted bases
 * are scored by base.  All device memory: base e of the set owns samples edges[e] .. edges[e + 1] - 1 (int64 [n_bases + 1], strictly
 * increasing from 0 to set_total) of labels and basemap (uint8 [set_total], as cf_label_events / cf_label_moves write them); stretch r
 * is length[r] samples from sample src_first[r] of the set, packed at bounds[r] of probs (float [total]); ranges (int64 [2][n]) holds
 * the first base at or behind the stretch's start and, n entries on, one past the last base that ends inside it.  With
 * q(p) = floor(double(p) * 2^32) (NaN and p < 0 count as 0, p > 1 as 1), per voted base of n samples:
 *   S          = the sum of q over its samples (uint64, exact)
 *   called_k   = S >= q(float(thresholds[k])) * n;   truth = labels[edges[e]] == 1;   class = A C G T / other of basemap[edges[e]] & 0x7f
 *   work       = sums uint64 [n_bases] | state uint8 [n_thresholds][n_bases] (bit 0 called, bit 1 truth, bits 2..4 class, bit 7 voted);
 *                zeroed by the call, so a base no stretch votes holds 0.  >= cf_base_votes_work_bytes(n_bases, n_thresholds), 8-byte aligned
 *   confusion_out  device int64 [n_thresholds][5][2][2] (class, truth, called) over the voted bases, zeroed and written by the call
 *   runs_out       device int64 [n_thresholds][2][3][5][max_bases + 1] (kind, state, class, bin), as cf_validation_run_bases lays it out: the
 *                  maximal streaks of voted bases of ONE stretch with truth (kind 0) or called (kind 1) set, judged against the other
 *                  bit; bin = min(bases, max_bases); zeroed and written by the call
 *   thresholds     HOST double [n_thresholds], 1..16 of them;  max_bases 1 .. 32;  longest_range a hint (the widest stretch in bases)
 * Two launches, asynchronous on `stream`, capturable; integer sums and integer atomics only, so equal inputs give equal bits whatever
 * the grid.  m may be NULL.  The tables are not trusted: ranges are clamped to [0, n_bases], a base whose samples are not
 * src <= edges[e] < edges[e + 1] <= src + length, inside the set and inside probs is unvoted (it breaks runs and is counted nowhere),
 * and nothing is read or written outside the buffers.  Stretches must not share a voted base.
 * CF_ERR_INVALID before any launch for a null pointer, a negative size, 2^31 or more stretches, samples or bases, n_thresholds outside
 * 1..16, max_bases outside 1..32 or a work buffer that is too small; n, n_bases, total or set_total == 0 is CF_OK with the tables zeroed. */
int64_t cf_base_votes_work_bytes(int64_t n_bases, int32_t n_thresholds);
int cf_base_votes(cf_model* m, const float* probs, int64_t total, const uint8_t* labels, const uint8_t* basemap, int64_t set_total,
                  const int64_t* edges, int64_t n_bases, const int64_t* src_first, const int64_t* length, const int64_t* bounds,
                  const int64_t* ranges, int64_t n, int64_t longest_range, const double* thresholds, int32_t n_thresholds, int32_t max_bases,
                  int64_t* confusion_out, int64_t* runs_out, void* work, int64_t work_bytes, void* stream);

/* Per-kernel device timing (HIP events on the launch stream) for bench.py's
 * roofline report.  cf_profile_enable(m, N) makes every N-th cf_infer call
 * (N = 1: every call; 0 = off) record events around each of its kernels; cf_profile_read synchronises and returns, for
 * kernel slot k, the accumulated milliseconds and launch count since the
 * last cf_profile_reset. */
#define CF_PROF_SLOTS 12
int cf_profile_enable(cf_model* m, int on);
int cf_profile_reset(cf_model* m);
int cf_profile_read(cf_model* m, double ms[CF_PROF_SLOTS], int64_t launches[CF_PROF_SLOTS]);
const char* cf_profile_slot_name(int slot);

/* Debug/test hook: copy an intermediate activation of the LAST pass to the
 * host in natural [n_windows, 35, features] order.  stage: 0..n_layers_res-1
 * = residual block outputs, n_layers_res + l = GRU layer l output (not
 * available for the last layer, whose output only exists as logits).  In the
 * bf16 precisions the stage is what the kernels stored: the value rounded to
 * bf16 (CF_PREC_BF16) or hi + lo of its split (CF_PREC_BF16X3). */
int cf_debug_stage(cf_model* m, int stage, int64_t n_windows, float* out_host);

/* Which card HIP device `device` of this process is -- the reference's per-file loop (catfish/catfish:50-82) shards over one
 * process per GPU, and each rank binds itself to the host CPUs next to ITS card (catfish_amd/placement.py) and says in the
 * benchmark line which card it drove.  pci_bus_id (>= 13 bytes, may be NULL) receives "dddd:bb:dd.f", the name of the
 * device's directory under /sys/bus/pci/devices (upper- or lower-case hex, as the runtime prints it); uuid_hex (>= 33 bytes,
 * may be NULL) the 16-byte device UUID as 32 hex digits.  Opens the HIP runtime (not a context on the device). */
int cf_device_identity(int device, char* pci_bus_id, int64_t bus_cap, char* uuid_hex, int64_t uuid_cap);

int64_t cf_workspace_bytes(const cf_model* m);
const char* cf_last_error(void);
const char* cf_version(void);
int cf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CATFISH_HIP_H */
