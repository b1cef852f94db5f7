/*
 * vp3d.h — C-ABI of the MI355X-native VideoPose3D temporal lifter.
 *
 * This is the drop-in boundary for the reference's hot path
 * (Bart-Weil/Dynamic-Camera-Augmented-VideoPose3D, common/models/TemporalModel.py).
 * The reference is pure Python, so it has no FFI of its own; every entry point
 * below names the Python interface it replaces (file:line in the reference) and
 * is bound from Python with ctypes.
 *
 * Conventions
 *   - Plain pointers and sizes only.  No torch types cross this boundary.
 *   - "device" pointers are HIP device allocations on the handle's device;
 *     "host" pointers are ordinary process memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 *   - Every function returns VP3D_OK (0) or a VP3D_ERR_* code; the message of the
 *     last failure on the calling thread is available from vp3d_last_error().
 *     The Python shim maps VP3D_ERR_ASSERT to AssertionError (the reference's
 *     `assert` convention, TemporalModel.py:21,63-65) and everything else to
 *     RuntimeError.
 *   - Layouts are channel-last: a (B, T, J, F) pose tensor is already the
 *     (B, T, J*F) activation matrix the first convolution consumes, and the
 *     (B, T', J_out*3) output matrix is already the (B, T', J_out, 3) result.
 */
#ifndef VP3D_H
#define VP3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VP3D_ABI_VERSION 1
#define VP3D_MAX_BLOCKS 8

/* status codes */
#define VP3D_OK 0
#define VP3D_ERR_ASSERT 1 /* shape / rank / config violation (reference: assert) */
#define VP3D_ERR_ARG 2    /* bad pointer or argument                          */
#define VP3D_ERR_HIP 3    /* HIP runtime failure                              */
#define VP3D_ERR_OOM 4    /* device allocation failed                         */
#define VP3D_ERR_STATE 5  /* handle misuse (wrong device, not reserved, ...)  */

/* model variants (TemporalModel.py:79 and :141) */
#define VP3D_VARIANT_DILATED 0    /* TemporalModel             */
#define VP3D_VARIANT_STRIDED_1F 1 /* TemporalModelOptimized1f  */

/* arithmetic type of the convolution stack */
#define VP3D_DTYPE_F32 0  /* exact f32 MFMA (v_mfma_f32_16x16x4_f32), the parity path */
#define VP3D_DTYPE_BF16 1 /* bf16 operands, f32 accumulate (v_mfma_f32_16x16x32_bf16) */
#define VP3D_DTYPE_F16 2  /* f16 operands, f32 accumulate (v_mfma_f32_16x16x32_f16)   */
/* split fp16: every f32 operand carried as hi + lo f16 halves (weights pre-scaled by a
 * per-layer power of two), each conv the three products hi.hi + hi.lo + lo.hi on
 * v_mfma_f32_16x16x32_f16 with f32 accumulation -- fp32-level results (the parity gate)
 * at the 16-bit MFMA rate; eval forward only (vp3d_forward / vp3d_forward_windows),
 * channels % 64 == 0 and <= 1024; the shrink runs the exact f32 GEMM */
#define VP3D_DTYPE_F16X3 3

/* Model configuration: the constructor arguments of TemporalModel /
 * TemporalModelOptimized1f (TemporalModel.py:85-86, :152-153). */
typedef struct vp3d_cfg {
    int32_t num_joints_in;
    int32_t in_features;
    int32_t num_joints_out;
    int32_t n_widths;                        /* len(filter_widths)                  */
    int32_t filter_widths[VP3D_MAX_BLOCKS];  /* odd widths, e.g. 3,3,3,3,3          */
    int32_t causal;                          /* 0/1                                 */
    int32_t channels;                        /* e.g. 1024                           */
    int32_t dense;                           /* 0/1 (dilated variant only)          */
    int32_t variant;                         /* VP3D_VARIANT_*                      */
    float bn_eps;                            /* BatchNorm1d eps (1e-5 in reference) */
} vp3d_cfg;

typedef struct vp3d_handle vp3d_handle;

/* ---- lifecycle (replaces TemporalModel.__init__ + load_state_dict + .cuda()) ---- */

/* Number of host weight arrays vp3d_create / vp3d_load_weights expect, in
 * state_dict order (TemporalModel.py:32-33,102,113-119):
 *   expand_conv.weight (C, J_in*F, w0)
 *   expand_bn.{weight, bias, running_mean, running_var} (C each)
 *   for i in 0..2*(n_widths-1)-1:
 *       layers_conv.i.weight (C, C, k_i)
 *       layers_bn.i.{weight, bias, running_mean, running_var}
 *   shrink.weight (J_out*3, C, 1), shrink.bias (J_out*3)
 * i.e. 5 + 10*(n_widths-1) + 2 arrays of float32, contiguous, PyTorch layout.
 * Returns the count, or -1 on an invalid configuration. */
int vp3d_weight_count(const vp3d_cfg* cfg);

/* Validate cfg (odd widths: TemporalModel.py:20-21), fold every eval-mode
 * BatchNorm into a per-channel (scale, shift) pair, pack the convolution
 * weights tap-major for the MFMA kernels (f32 and bf16 copies) and upload them
 * to the current HIP device.  `weights` are HOST pointers. */
int vp3d_create(const vp3d_cfg* cfg, const float* const* weights, int n_weights, vp3d_handle** out);

/* Re-pack and re-upload weights into an existing handle (load_state_dict,
 * TemporalModel.py via nn.Module; called by run.py:416-417). Synchronous. */
int vp3d_load_weights(vp3d_handle* h, const float* const* weights, int n_weights);

int vp3d_destroy(vp3d_handle* h);

/* ---- shape helpers (TemporalModel.py:40-60) ---- */
int vp3d_receptive_field(const vp3d_handle* h);     /* 1 + 2*sum(pad)               */
int vp3d_total_causal_shift(const vp3d_handle* h);  /* bit-compatible, quirk Q5     */
/* Output frames for an input of T frames, or -1 if T is invalid for the variant. */
int vp3d_out_frames(const vp3d_handle* h, int T);

/* ---- forward (replaces TemporalModelBase.forward, TemporalModel.py:62-76) ---- */

/* Allocate the activation workspace for (B, T, dtype) up front so that a later
 * vp3d_forward with B' <= B, T' <= T allocates nothing (and can be captured into
 * a hipGraph). */
int vp3d_reserve(vp3d_handle* h, int B, int T, int dtype);

/* Eval-mode forward.  x: device f32 (B, T, J_in, F) contiguous.
 * y: device f32 (B, vp3d_out_frames(T), J_out, 3) contiguous, written here.
 * Launches on `stream`; returns without synchronising. */
int vp3d_forward(vp3d_handle* h, const float* x, int B, int T, float* y, int dtype, void* stream);

/* Synchronise `stream` and report a device-side fault of this handle's launches since the
 * last call: VP3D_ERR_STATE when a split-K owner tile (conv_gemm_a4, the partial last round
 * of small f16x3 batches) gave up waiting for its helper units -- its output was then
 * wrong -- or when an f16x3 forward split a value past the f16 range of its halves
 * (|x| > 65,504: checked where the input rows and every hidden activation are split) or
 * produced non-finite poses (run such inputs in fp32), or when a pair of an expand-table
 * forward (vp3d_forward_windows_pool) named a sequence outside the pool; the fault is cleared by this call.  (The next vp3d_forward* on the handle also
 * refuses with VP3D_ERR_STATE while the fault is pending, without synchronising -- every
 * dtype after a split-K timeout, f16x3 only after an f16x3 range fault.)  No
 * reference counterpart: torch raises asynchronous device errors at the next sync. */
int vp3d_sync_status(vp3d_handle* h, void* stream);

/* Eval-mode forward of B windows gathered on the fly from device-resident
 * sequences: the ChunkedGenerator batch (generators.py:102-137; edge padding of
 * pad_chunk :92-100) and the trajectory concat (CamTransformer.py:187-190) feeding
 * TemporalModelBase.forward (TemporalModel.py:62-76) without materialising the
 * (B, window, J_in*F) input.  On the 16-bit path the gather is fused into the
 * expand conv's operand loads; otherwise the windows go through a scratch tensor.
 *   kps:     device f32 (n_frames, f2) normalised keypoints of all sequences
 *   cams:    device f32 (n_frames, 12) per-frame K.E, or NULL (no concat);
 *            f2 (+ 12) must equal num_joints_in * in_features
 *   seq_off: device int64 first frame of each sequence; seq_len: device int32
 *   pairs:   device int32 (B, 2) = (sequence, start); window b = sequence frames
 *            [start - lead, start - lead + window), clamped to [0, len-1]
 *   y:       device f32 (B, vp3d_out_frames(window), J_out, 3)
 * With cams, dtype VP3D_DTYPE_BF16 is refused (VP3D_ERR_ARG): its 8-bit mantissa on the
 * metre-scale K.E channels costs ~30 mm; fp16, f16x3 (the accurate fast path) or f32. */
int vp3d_forward_windows(vp3d_handle* h, const float* kps, int32_t f2, const float* cams,
                         const int64_t* seq_off, const int32_t* seq_len, const int32_t* pairs, int B,
                         int window, int lead, float* y, int dtype, void* stream);

/* vp3d_forward_windows with the resident pool described: `n_seq` sequences (the entries of
 * seq_off / seq_len that pairs may name), the longest of `max_len` frames.  The same poses, bit
 * for bit.  Knowing the pool lets an f16x3 forward without the camera concat compute the expand
 * conv (TemporalModel.py:126-127, :188-189) once per resident frame instead of once per window
 * row -- its output depends on the sequence and the frame position alone -- into a table of
 * n_seq * T_tab rows (T_tab = max_len + lead + twice the frames a window's rows step over, rounded
 * up to 16: every window start, in or outside its sequence, maps to rows with its edge clamp)
 * that block 1 reads through per-window row bases.  Taken, from the sizes alone, when the table
 * has at most half the rows of the per-window expand output (n_seq * T_tab <= B * rows / 2), is
 * smaller than 2 GiB and both block-1 convs run the tile kernels that read indirect rows
 * (conv_gemm_a4: 1,024-channel shapes); otherwise the call is vp3d_forward_windows exactly.  Large evaluation
 * batches over a resident set qualify; a training-size batch over a large set never does.
 * VP3D_EXPAND_TABLE (read once per forward): 0 = never, 1 = whenever the table fits 2 GiB,
 * copy = the table, then the windows' rows copied out of it for block 1 (also what block-1
 * kernel forms without indirect rows get).
 * Frame tables: the same holds below the point where windows stop overlapping -- row j of block
 * b's output in the window starting at frame s depends on the sequence and on frame position
 * s + step j alone -- so with the expand table read through indirect rows, blocks 1 .. d are
 * computed once per table row as well (one dilated launch per layer over the level below, three
 * table-sized buffers rotating), and block d + 1 is the first per-window block, reading level d
 * through the window bases.  The depth d is the deepest, at most blocks - 1, for which at every
 * level the table a block reads has at most half that block's window rows, its launches run
 * conv_gemm_a4's whole / half-N / quarter-N tiles (never a split-K form: every table row keeps the
 * K order of the window row it replaces) and block d + 1 reads indirect rows; the poses are the
 * same bits at every depth.  VP3D_FRAME_TABLES=<d> (read once per forward) forces a depth, also
 * past the size rule, clamped to what the other conditions allow: 0 = the expand table only, d >= 1
 * takes the expand table with it unless VP3D_EXPAND_TABLE is 0 or copy.
 * The size rule, for the expand table and every level alike (vp3d_table_depth_rule): "at most half"
 * where the table's launch is shorter than one round of 256 x 256 tiles; where it is at least one
 * round, the measured rule -- nominal table rows <= the window rows (ratio 1).  Nominal rows are
 * n_seq * T_tab as above, whichever rows are then computed:
 * Trimmed layout: window starts that generators make lie in [0, len), so by default the tables
 * hold the rows of the starts 0 .. max_len - 1 only (max_len + the frames a window steps over,
 * rounded up to 16, per sequence: 14 % fewer than T_tab at max_len 2,048, lead 121).  Starts before
 * frame 0 or from max_len on stay exact: two edge segments per sequence hold their rows, filled by
 * launches that are enqueued with every forward and return at entry unless that forward's batch
 * holds such a start (decided on the device: no host synchronisation).  A forward whose batch did
 * makes the next forward on the handle take the wide layout (one region for every start, no edge
 * segments: fewer rows than main + edges) until a batch without such starts has been seen.
 * VP3D_TABLE_TRIM=0|1 (read once per forward) forces wide or trimmed; vp3d_table_layout reports.
 * Clamp-constant edge rows: a main-region row of level l >= 1 whose frames all lie at or before
 * frame 0, or all at or after frame max_len - 1, holds the same value as its neighbour towards the
 * sequence in every sequence (frames clamp to the sequence's first / last one), so each level's
 * launches compute the rows a_l .. b_l between those runs only and a small copy kernel fills the
 * rest from rows a_l and b_l -- the same bits (113 / 95 / 41 rows per side of levels 1 / 2 / 3 at
 * max_len 2,048, lead 121).  VP3D_TABLE_EDGES=0|1 (read once per forward; default 1) turns that
 * off / on; a level whose shortened launch would leave the a4 tile forms keeps its full rows;
 * vp3d_table_rows reports.
 * A forward that takes a table must not be captured into a hipGraph: its launches carry the
 * forward's serial number as an argument, and a replay after a later forward on the handle would
 * skip the edge launches its own bases may point into (graph capture is vp3d_forward's only).
 * What differs from vp3d_forward_windows on this path:
 *   - the f16x3 range guard (vp3d_sync_status) sees every table row computed at every level --
 *     frame positions of the n_seq sequences whether or not a window uses them; in the trimmed
 *     layout not the rows of starts outside 0 .. max_len - 1 unless the batch holds such a start
 *     -- so one non-finite resident frame, or an activation past the f16 range at a frame
 *     position no window reads, faults the forward;
 *   - a pair naming a sequence outside [0, n_seq) is a fault reported by vp3d_sync_status /
 *     the next forward (window starts outside their sequence are edge-clamped as ever). */
int vp3d_forward_windows_pool(vp3d_handle* h, const float* kps, int32_t f2, const float* cams,
                              const int64_t* seq_off, const int32_t* seq_len, int32_t n_seq, int32_t max_len,
                              const int32_t* pairs, int B, int window, int lead, float* y, int dtype,
                              void* stream);
/* The path the handle's last gathered forward took: 0 = the expand conv per window row, 1 = the
 * expand table read by block 1 through indirect rows, 2 = the table with the windows' rows
 * copied out.  -1 for a NULL handle.  (Diagnostics and tests.) */
int vp3d_expand_table_mode(const vp3d_handle* h);
/* The frame-table depth of the handle's last gathered forward: the blocks computed once per table
 * row (0 = none: the expand table at most).  -1 for a NULL handle.  (Diagnostics and tests.) */
int vp3d_frame_table_depth(const vp3d_handle* h);
/* Which table rows the handle's last gathered forward computed: 0 = no table, 1 = the wide
 * layout (every start lo .. max_len - 1 + lead in one region per sequence), 2 = the trimmed layout
 * (the starts 0 .. max_len - 1, the others in gated edge segments).  *edges (may be NULL): 1 when
 * that forward's batch held a start outside 0 .. max_len - 1 after the edge clamp -- in the trimmed
 * layout, when its edge gate fired; valid once the forward has completed (synchronise first).
 * -1 for a NULL handle.  (Diagnostics and tests.) */
int vp3d_table_layout(const vp3d_handle* h, int* edges);
/* The main-region rows of table level `level` (0 = the expand table, l = block l's output, up to
 * vp3d_frame_table_depth) that the convs of the handle's last gathered forward computed, per
 * sequence: rows *first_row .. *first_row + *rows - 1 of the *pitch rows a sequence has at that
 * level; the rows outside are copies of the first / last computed row (clamp-constant edge rows,
 * above).  *rows == *pitch: every row computed.  Each pointer may be NULL.  VP3D_OK, or
 * VP3D_ERR_ARG for a NULL handle or a level the forward had no table of.  (Diagnostics and tests.) */
int vp3d_table_rows(const vp3d_handle* h, int level, int* first_row, int* rows, int* pitch);
/* The size rule of the table paths: a table (the expand table, each frame-table level) is taken
 * when its nominal rows are at most 1 / *factor of the window rows it replaces where its launch is
 * shorter than one round of 256 x 256 tiles, and at most *ratio_num / *ratio_den of them where it
 * is at least one round.  (Diagnostics and tests.) */
void vp3d_table_depth_rule(int* factor, int* ratio_num, int* ratio_den);

/* ---- f16x3 activation pre-scale (opt-in; no reference counterpart) ----
 * The split-fp16 path stores every activation as hi = f16(a), lo = f16(a - hi); lo is an f16
 * subnormal for |a| < 2^-3, an absolute floor of 2^-25 per stored value, so a checkpoint whose
 * hidden activations are small loses accuracy silently.  An exact power-of-two pre-scale per
 * conv layer output moves the stored rows back into range: layer l's stored rows hold
 * a * 2^p[l], folded into the f16x3 epilogue's scale and shift when the weights are packed
 * (the eval BatchNorm + ReLU of TemporalModel.py:102-119 commute with a positive scale), the
 * next layer absorbing the inverse and the shrink (TemporalModel.py:75) the last one.  Nothing
 * changes per forward; the fp32 / bf16 / fp16 paths never see it. */
#define VP3D_X3_PRESCALE_MAX 24

/* Set one exponent per conv layer output: n = vp3d_layer_count(h) - 1 (the shrink has none),
 * in layer order (expand, then k-conv and 1x1 of each block, TemporalModel.py:102-119).  The
 * residual add (TemporalModel.py:132 / :192) joins the expand output and every block's 1x1
 * output, so layers 0, 2, 4, ... must share one exponent ("the chain"); each k-conv output
 * (layers 1, 3, ...) has its own.  VP3D_ERR_ARG (vp3d_last_error names the layer) for a vector
 * that breaks this, for |p| > VP3D_X3_PRESCALE_MAX, or for a wrong n.  All zeros restores the
 * unscaled state bit for bit.  Kept across vp3d_load_weights.  Synchronises the device when
 * the exponents change.  A pre-scale that pushes a stored value past 65,504 is caught by the
 * f16x3 range guard (vp3d_sync_status). */
int vp3d_set_x3_prescale(vp3d_handle* h, const int32_t* p, int n);
int vp3d_get_x3_prescale(const vp3d_handle* h, int32_t* p, int n);

/* Per-layer statistics of the calibration pass. */
typedef struct vp3d_act_stats {
    double absmax;      /* max |a| over the layer's output; inf / NaN if one occurred        */
    double rms;         /* sqrt(mean a^2), summed in f64                                      */
    double small_share; /* share of the values with a != 0 and |a| < 2^-3 (subnormal lo half) */
} vp3d_act_stats;

/* Calibration: run the fp32 forward (TemporalModel.py:62-76) on x (device f32, (B, T, J_in, F))
 * and reduce every conv layer's output on the device (after BN, ReLU and the residual add of
 * TemporalModel.py:102-119,126-138 -- the values the f16x3 path stores) into
 * stats_out[0 .. vp3d_layer_count(h) - 2], a HOST array.  The fp32 path measures, never the
 * f16x3 one (it is the degraded thing being measured); the handle's pre-scale is neither
 * read nor changed.  Synchronous. */
int vp3d_x3_calibrate(vp3d_handle* h, const float* x, int B, int T, vp3d_act_stats* stats_out, void* stream);
/* The same on windows gathered from device-resident sequences (arguments as
 * vp3d_forward_windows; generators.py:102-137, CamTransformer.py:187-190). */
int vp3d_x3_calibrate_windows(vp3d_handle* h, const float* kps, int32_t f2, const float* cams,
                              const int64_t* seq_off, const int32_t* seq_len, const int32_t* pairs, int B,
                              int window, int lead, vp3d_act_stats* stats_out, void* stream);

/* ---- per-layer timing (HIP events recorded on the launch stream) ---- */
int vp3d_profile_enable(vp3d_handle* h, int enable);
/* Restrict the timing to the layers in `mask` (bit i = layer i; all by default), e.g.
 * only the dominant layer inside a timed loop so the other launches carry no events. */
int vp3d_profile_layers(vp3d_handle* h, uint64_t mask);
/* Number of kernel launches one forward makes (conv layers incl. shrink). */
int vp3d_layer_count(const vp3d_handle* h);
/* Accumulated time (ms) and launch count per layer since the last reset, and
 * the algorithmic FLOP of each layer's most recent launch.  Synchronises on
 * the recorded events.  Arrays have vp3d_layer_count() entries. */
int vp3d_profile_read(vp3d_handle* h, double* ms_total, int64_t* launches, double* flop_last);
int vp3d_profile_reset(vp3d_handle* h);

/* ---- causal streaming (BASELINE config 5) ----
 * One frame in, one pose out, for a causal dilated model (TemporalModel with
 * causal=True, TemporalModel.py:107-111): every convolution is a GEMV over taps
 * read from per-layer ring buffers of past activations.  Output k equals frame k
 * of the reference's whole-sequence causal evaluation (UnchunkedGenerator edge
 * padding, generators.py:193-198).  The stream position lives in device memory,
 * so one step is replayable from a hipGraph. */
typedef struct vp3d_stream vp3d_stream;

/* dtype: VP3D_DTYPE_* of the weights streamed per step (f16 in config 5; F32 keeps the
 * exact fp32 weights resident, the north-star accuracy form). */
int vp3d_stream_create(vp3d_handle* h, int dtype, vp3d_stream** out);
/* Restart the stream (the next frame is frame 0).  Async on `stream`. */
int vp3d_stream_reset(vp3d_stream* s, void* stream);
/* Device frame queue and pose ring of the stream (queue_len slots each, a power of
 * two): step t reads frame slot t % queue_len and writes pose slot t % queue_len.
 * Graph replays read/write exactly these; frames can be queued ahead of time. */
int vp3d_stream_io(vp3d_stream* s, float** in_frames, float** out_poses, int* queue_len);
/* One step.  frame / pose: device pointers (frame copied into the queue slot of
 * this step, pose copied out of it, asynchronously), or NULL to use the queue
 * slot as is. */
int vp3d_stream_step(vp3d_stream* s, const float* frame, float* pose, void* stream);
/* Frames consumed so far (synchronises with the device). */
int64_t vp3d_stream_frames_seen(vp3d_stream* s);
/* Capture `steps` consecutive steps (frames from the queue) into a hipGraph on
 * `stream` (not the legacy default stream); replay with vp3d_stream_graph_launch. */
int vp3d_stream_graph_capture(vp3d_stream* s, void* stream, int steps);
int vp3d_stream_graph_launch(vp3d_stream* s, void* stream);
int vp3d_stream_destroy(vp3d_stream* s);
/* 1 when the stream runs as one persistent launch per batch of steps (weights resident
 * on chip, layer outputs handed between CUs in-launch), 0 for one GEMV launch per layer
 * (VP3D_STREAM_MODE=launches at vp3d_stream_create, or a shape no persistent form takes). */
int vp3d_stream_persistent(const vp3d_stream* s);
/* Form of the in-launch step: 2 = layer-pipelined (stream_pipe.hip: each CU runs one
 * layer with its weights in VGPRs, frames of a batch pipelined through the layer groups;
 * the default at 1024 / 256 channels with 3-tap blocks, f32 weights held as they are,
 * 16-bit ones widened to f32), 1 = every CU runs every layer with its 16-bit weights in LDS
 * (stream_persist.hip), 0 = one GEMV launch per layer.  VP3D_STREAM_MODE=pipe|persist|launches at vp3d_stream_create restricts it. */
int vp3d_stream_mode(const vp3d_stream* s);
/* Synchronises; VP3D_ERR_STATE if a persistent launch gave up waiting on another CU
 * (bounded spins: the grid did not fit the device at once), else VP3D_OK. */
int vp3d_stream_status(vp3d_stream* s);

/* ---- serving: one frame in flight, real time (config 5's single-frame latency) ----
 * The layer-pipelined launch (mode 2) stays resident with its weights in VGPRs and takes
 * frames as the host posts them through pinned host memory; the pose of frame t comes back
 * the same way, with no launch, copy or graph per frame.  The launch ends by itself at
 * the first frame not posted within idle_ms, or at vp3d_stream_serve_end.  Frames keep
 * the stream's numbering (the first posted frame is frame vp3d_stream_frames_seen()).
 * At most queue_len - 1 frames may be posted and not yet waited for.
 * The last block's 1x1 workgroups fold the shrink in (VP3D_STREAM_FOLD, default on): each
 * stores its channels' partial pose sums and the host adds them in a fixed order (one layer
 * group fewer on the frame's path: median 24.4 vs 25.4 us), so served poses equal the batch
 * form's within 1e-6 m, not bit for bit; the host-side shrink affine is re-read from the
 * handle at every serve_begin (after vp3d_load_weights too).  hipFree / hipDeviceSynchronize anywhere in the
 * process wait for the resident launch (it ends at idle_ms): end serving before freeing
 * device memory or destroying another stream.
 */
int vp3d_stream_serve_begin(vp3d_stream* s, void* stream, double idle_ms);
/* Copy one frame (host f32, J_in * F values) into the ring and post it; *frame_index is
 * its stream index.  VP3D_ERR_STATE when not serving, the ring is full or the launch ended. */
int vp3d_stream_serve_post(vp3d_stream* s, const float* frame, int64_t* frame_index);
/* Wait (spinning on host memory, at most timeout_ms) until frame `frame_index` is done and
 * copy its pose (host f32, J_out * 3) out.  VP3D_ERR_STATE on timeout or stream fault. */
int vp3d_stream_serve_wait(vp3d_stream* s, int64_t frame_index, float* pose, double timeout_ms);
/* post + wait in one call (one frame in flight); *latency_us (or NULL) = host wall time from
 * the start of the post to the pose copied out. */
int vp3d_stream_serve_step(vp3d_stream* s, const float* frame, float* pose, double timeout_ms, double* latency_us);
/* Stop serving: the launch finishes the posted frames and exits; synchronises `stream`. */
int vp3d_stream_serve_end(vp3d_stream* s, void* stream);
/* Diagnostics of the layer-pipelined form (no reference counterpart): with VP3D_STREAM_TRACE=n
 * set at vp3d_stream_create, every workgroup records the 100 MHz device clock when the input of
 * each of the first n frames of a launch is complete and, per wave, after the wave's first
 * output store.  Copies workgroups x n x 11 clocks ([0] input complete, [1 + w] wave w stored;
 * [9], [10]: the shader clock counter at [0] and [1]) to `out` (NULL: sizes only) and clears them; role_first_wg (n_roles
 * + 1 entries, or NULL) = the first workgroup of each layer role (expand, k / 1x1 per block,
 * shrink).  Synchronises the device. */
int vp3d_stream_trace(vp3d_stream* s, uint64_t* out, int64_t capacity, int32_t* role_first_wg, int32_t* n_roles,
                      int32_t* frames);

/* ---- batched causal streaming: many streams advance in one step ----
 * n_streams independent causal streams ("slots") of one model, each with its own position
 * and its own rings, advanced together: every layer of a step is one skinny GEMM (slots x K
 * by K x channels, exact f32 MFMA, f32 activations; 16-bit weights widened in registers), so
 * the weights are read once per step however many slots take part (stream_batch.hip).  Slot
 * s's k-th active step equals frame k of the reference's whole-sequence causal evaluation of
 * the frames that slot consumed (TemporalModel.py:79-138 with causal=True, UnchunkedGenerator
 * edge padding, generators.py:193-198), as for a vp3d_stream.  The single stream above
 * remains the one-stream path. */
#define VP3D_MSTREAM_MAX 64
typedef struct vp3d_mstream vp3d_mstream;

/* Accepts what the per-layer-launch form of vp3d_stream_create accepts (a causal dilated or
 * dense TemporalModel, K <= 4096 per layer, dtype F32 / F16 / BF16) with the same status
 * codes, and 1 <= n_streams <= VP3D_MSTREAM_MAX (else VP3D_ERR_ARG).  Shares the handle's
 * device weights: a vp3d_load_weights is seen by the next step. */
int vp3d_mstream_create(vp3d_handle* h, int dtype, int n_streams, vp3d_mstream** out);
/* The device io buffers a step reads / writes: frames (S, J_in * F) f32, active (S) int32
 * (nonzero = the slot consumes its frame in this step), poses (S, J_out * 3) f32. */
int vp3d_mstream_io(vp3d_mstream* m, float** frames, int32_t** active, float** poses);
/* One step of every active slot (the reference's model(inputs_2d) on each slot's next frame,
 * run.py:689-724, one frame at a time).  frames / active / poses: device pointers copied into
 * / out of the io buffers asynchronously, or NULL to use the io buffers as they are; active
 * == NULL with frames != NULL means every slot is active.  An inactive slot stores nothing:
 * no ring slot, no position change, and its pose row keeps the value of its last active step. */
int vp3d_mstream_step(vp3d_mstream* m, const float* frames, const int32_t* active, float* poses, void* stream);
/* Restart slot `slot` (-1 = every slot): its next frame is frame 0 (a new sequence through
 * the reference's generator).  Async on `stream`; rings are not cleared (step 0 rewrites
 * time 0 before any tap reads it). */
int vp3d_mstream_reset(vp3d_mstream* m, int slot, void* stream);
/* Frames consumed so far by each slot (host array of n_streams entries; synchronises with
 * the device). */
int vp3d_mstream_frames_seen(vp3d_mstream* m, int64_t* out);
/* Capture one step (reading / writing the io buffers) into a hipGraph on `stream` (not the
 * legacy default stream): a linear chain of kernel nodes.  Replay with
 * vp3d_mstream_graph_launch. */
int vp3d_mstream_graph_capture(vp3d_mstream* m, void* stream);
int vp3d_mstream_graph_launch(vp3d_mstream* m, void* stream);
int vp3d_mstream_destroy(vp3d_mstream* m);

/* ---- look-ahead streaming: non-causal models on live tracks, batched, with drain ----
 * The batched step above for a NON-causal TemporalModel (TemporalModel.py:79-138 with
 * causal=False, the reference's default and what its 243-frame checkpoints are).  A non-causal
 * dilated stack is the causal stack seen lookahead = (receptive field - 1) / 2 frames late: in
 * arrival time every layer still reads taps at t - (taps-1-k) * dilation, clamped at the stream
 * start; a block's residual is the centre tap of its k-conv window (TemporalModel.py:132 with
 * causal_shift = 0), the block input pad_b steps back; and the end of a sequence is edge-padded
 * on the right as well (UnchunkedGenerator, generators.py:193-198: (pad, pad) copies), which a
 * slot gets by draining.  Pose k of a slot equals frame k of the reference's whole-sequence
 * evaluation (run.py:689-724, evaluate() on one UnchunkedGenerator sequence) of the n frames
 * the slot consumed.
 *
 * Per step every slot gets a code: 0 idle, 1 consume its frame, 2 drain (a step whose new frame
 * repeats the slot's last consumed one); any other value is idle.  A slot counts n, the frames
 * consumed, and t, the steps taken (consume + drain).  A step with t >= lookahead writes the pose
 * of frame t - lookahead into the slot's pose row; earlier steps run every layer (the rings
 * fill) but write no row, and a row that is not written keeps its content (zeros at first).
 * After n frames and `lookahead` drains a slot has emitted exactly n poses.  No-ops -- nothing
 * stored, no counter changed, pose_frame -1: a drain with n == 0 or with n poses emitted, and a
 * consume once the slot has drained (until it is reset). */
typedef struct vp3d_lstream vp3d_lstream;

/* Accepts a non-causal dilated or dense TemporalModel (TemporalModel.py:79-138), K <= 4096 per
 * layer, dtype F32 / F16 / BF16, 1 <= n_streams <= VP3D_MSTREAM_MAX; VP3D_ERR_ARG with a message
 * otherwise (a causal model: "look-ahead 0: use vp3d_mstream"; the strided
 * TemporalModelOptimized1f, :141-198; other dtypes).  Shares the handle's device weights. */
int vp3d_lstream_create(vp3d_handle* h, int dtype, int n_streams, vp3d_lstream** out);
/* The look-ahead in frames: the sum of the layers' pads (TemporalModel.py:31,107-111), 121 at
 * receptive field 243. */
int vp3d_lstream_lookahead(vp3d_lstream* l, int32_t* out);
/* The device io buffers a step reads / writes: frames (S, J_in * F) f32, codes (S) int32,
 * poses (S, J_out * 3) f32, pose_frame (S) int32 -- the frame index of the pose row the last
 * step wrote for the slot, or -1 (generators.py:193-198: frame k of the padded sequence's
 * output). */
int vp3d_lstream_io(vp3d_lstream* l, float** frames, int32_t** codes, float** poses, int32_t** pose_frame);
/* One step (the reference's model(inputs_2d), run.py:689-724, one frame at a time and
 * `lookahead` frames late).  frames / codes / poses / pose_frame: device pointers copied into /
 * out of the io buffers asynchronously, or NULL to use the io buffers as they are; codes == NULL
 * with frames != NULL means every slot consumes. */
int vp3d_lstream_step(vp3d_lstream* l, const float* frames, const int32_t* codes, float* poses, int32_t* pose_frame,
                      void* stream);
/* Restart slot `slot` (-1 = every slot) for a new sequence through the reference's generator
 * (generators.py:193-198): frames consumed, steps taken, poses emitted and the drained state go
 * to 0.  Async on `stream`; rings and pose rows are not cleared. */
int vp3d_lstream_reset(vp3d_lstream* l, int slot, void* stream);
/* Frames consumed and poses emitted so far by each slot (host arrays of n_streams entries,
 * either may be NULL; synchronises with the device).  A sequence of the reference's generator
 * (generators.py:193-198) is done when emitted == consumed. */
int vp3d_lstream_counts(vp3d_lstream* l, int64_t* consumed, int64_t* emitted);
/* Capture one step (reading / writing the io buffers, pose_frame included; run.py:689-724 per
 * frame) into a hipGraph on `stream` (not the legacy default stream); replay with
 * vp3d_lstream_graph_launch. */
int vp3d_lstream_graph_capture(vp3d_lstream* l, void* stream);
/* Replay the captured step on `stream`: one model(inputs_2d) per slot (run.py:689-724) on the
 * frames and codes in the io buffers; VP3D_ERR_STATE without a captured graph. */
int vp3d_lstream_graph_launch(vp3d_lstream* l, void* stream);
/* Free the slots' rings, io buffers and graph; the handle and its weights (the TemporalModel's,
 * TemporalModel.py:79-138) stay.  NULL is VP3D_OK. */
int vp3d_lstream_destroy(vp3d_lstream* l);

/* ---- training step (run.py:451-487, :662) ----
 * The reference trains TemporalModel in train mode: BatchNorm1d on batch
 * statistics with a running-stat update (TemporalModel.py:117,119; momentum
 * decayed per epoch by set_bn_momentum :35-38, run.py:553-556), ReLU, Dropout
 * (:130-137), the residual add, then loss.backward() and
 * optim.Adam(amsgrad=True).step().  A trainer runs that forward/backward on the
 * device in f32.  Parameters stay in caller-owned device memory (the
 * nn.Module's own tensors) and are passed per call as a table of device
 * pointers in state_dict order — the same order and count as vp3d_create's
 * `weights` (vp3d_weight_count): conv weight, then BN weight / bias /
 * running_mean / running_var per conv, shrink weight and bias.  Dropout masks
 * come from a counter-based hash of (seed, layer, element), regenerated in the
 * backward rather than stored (vp3d_train_dropout_mask exports them). */
typedef struct vp3d_trainer vp3d_trainer;

int vp3d_trainer_create(const vp3d_cfg* cfg, vp3d_trainer** out);
int vp3d_trainer_destroy(vp3d_trainer* t);

/* Train-mode forward (TemporalModelBase.forward in train mode, TemporalModel.py:62-76).
 * params: host array of n_params DEVICE pointers (state_dict order); the BN
 * running_mean / running_var entries are updated in place with `momentum`
 * (BatchNorm1d.momentum).  x: device f32 (B, T, J_in, F); y: device f32
 * (B, vp3d_out_frames(T), J_out, 3).  dropout_p: nn.Dropout p; seed: mask seed.
 * The activations the backward needs are kept inside the trainer until the next
 * forward. */
int vp3d_train_forward(vp3d_trainer* t, float* const* params, int n_params, const float* x, int B, int T,
                       float dropout_p, double momentum, uint64_t seed, float* y, void* stream);

/* Backward of the latest vp3d_train_forward (same params, which must not have
 * changed in between).  dy: device f32 like y.  grads: host array of n_params
 * device pointers, state_dict order; each trainable entry receives its gradient
 * (overwritten, torch layout); running-stat entries are ignored and may be NULL.
 * The input gradient is not formed (the 2D keypoints are data, run.py:458). */
int vp3d_train_backward(vp3d_trainer* t, float* const* params, int n_params, const float* dy,
                        float* const* grads, void* stream);

/* The dropout keep mask (1 = kept) of conv layer `layer` (0 = expand, then the
 * block convs in order) for the latest forward: n_elems = rows * channels of that
 * layer's output, row-major (b, t, c).  Test hook for the parity tests. */
int vp3d_train_dropout_mask(vp3d_trainer* t, int layer, int64_t n_elems, uint8_t* out, void* stream);

/* The ReLU mask (1 = BN output > 0) of conv layer `layer` in the latest forward, same
 * layout as vp3d_train_dropout_mask.  Test hook: an element whose BN output lies within
 * rounding of 0 may take the other side of the ReLU in another f32 implementation, so the
 * parity tests feed this mask (with the dropout mask) to the oracle. */
int vp3d_train_relu_mask(vp3d_trainer* t, int layer, int64_t n_elems, uint8_t* out, void* stream);

/* Mixed-precision training.  dtype: VP3D_DTYPE_F32 (the default: every GEMM on the exact-f32
 * MFMA) or VP3D_DTYPE_BF16; anything else is VP3D_ERR_ARG (fp16 / f16x3 training would need
 * loss scaling: the gradients of a mean-over-batch MPJPE lie far below f16's range).  In bf16
 * mode the three GEMMs of every BLOCK convolution (conv layers 1 .. n-2: each block's k-conv
 * and its 1x1) take bf16 operands, each rounded to nearest even from the f32 value the f32
 * step uses, and accumulate in f32:
 *   forward          Z[l]  = conv(bf16(Out[l-1]), bf16(W[l]))
 *   data gradient    dX    = conv^T(bf16(dZ[l]), bf16(W[l]))
 *   weight gradient  dW[l] = bf16(dZ[l])^T x gather(bf16(Out[l-1]))
 * The expand conv (2D coordinates in) and the shrink (metre-scale poses out) keep the f32 path
 * in every role; BatchNorm statistics, the BN / ReLU / dropout / residual passes, the gradients
 * handed back, the parameters and Adam stay f32.  The weights are re-rounded from the f32
 * parameters on every forward and backward call.  channels % 8 != 0 is VP3D_ERR_ARG in bf16
 * mode (the 16-bit rows are read 8 elements at a time).  The setting holds from the next
 * forward; a backward whose forward ran under another setting is VP3D_ERR_STATE. */
int vp3d_trainer_set_compute(vp3d_trainer* t, int dtype);
/* The setting of vp3d_trainer_set_compute (-1 for NULL). */
int vp3d_trainer_compute(const vp3d_trainer* t);

/* Test hooks for the parity tests of the bf16 mode (small shapes only: extra memory).
 * vp3d_train_capture(t, on): while on, every backward keeps, per conv layer, a dense f32 copy
 * of the gradient rows that layer's dgrad and wgrad consumed (what `which` = 1 returns).
 * vp3d_train_read(t, layer, which, out, n, stream), for the latest forward / backward:
 *   which = 0  the rows conv `layer` consumed as its activation operand: B * (input frames of
 *              the layer) rows of cin values (layer 0: x itself, read through the forward's
 *              pointer, which the caller must still hold)
 *   which = 1  the gradient rows its dgrad and wgrad consumed: B * (output frames) rows of
 *              cout values, without the dgrad's zero padding (the shrink: dy); needs capture
 * In bf16 mode the rows of a block conv are the bf16 operands widened to f32 (exact); otherwise
 * the f32 rows.  out: device f32, n = rows * width.  VP3D_ERR_STATE without a forward, or
 * (which = 1) without capture on during the latest backward; VP3D_ERR_ARG for a wrong n,
 * layer or which. */
int vp3d_train_capture(vp3d_trainer* t, int on);
int vp3d_train_read(vp3d_trainer* t, int layer, int which, float* out, int64_t n, void* stream);

/* Measurement (tools/bench_train_dtype.py).  Synchronises the device; if `ms` is not NULL it
 * receives the device time, in milliseconds and summed since the previous call, of four roles
 * of the forwards and backwards run with profiling on: [0] forward conv GEMMs, [1] data-gradient
 * GEMMs, [2] weight gradients (tiles + split reduce), [3] the element-wise / per-channel passes
 * (weight packs, BatchNorm, ReLU / dropout / residual, column sums).  Then profiling is switched
 * on or off.  While on, every launch group is bracketed by two events (a little slower). */
int vp3d_train_profile(vp3d_trainer* t, int on, double* ms);

/* Row count (B * frames) of conv layer `layer`'s output in the latest forward, or -1. */
int64_t vp3d_train_layer_rows(const vp3d_trainer* t, int layer);

/* Doubles of per-channel partial sums (two per channel and row chunk) of a column reduction
 * over `rows` rows of `channels`: reserved = 0, what a reduction over exactly `rows` rows
 * writes; reserved = 1, what a trainer sized for `rows` rows reserves, a bound over every row
 * count up to `rows` (the chunk count is not monotone in the row count).  Host arithmetic only;
 * test hook.  -1 for a negative row count or channels <= 0. */
int64_t vp3d_train_reduce_doubles(int64_t rows, int channels, int reserved);

/* One Adam step over n tensors (torch.optim.Adam, _single_tensor_adam; run.py:662
 * builds it with amsgrad=True): for each i, with g = grad (+ weight_decay * param),
 *   exp_avg = lerp(exp_avg, g, 1 - beta1)   (as fma, like ATen's vectorised lerp)
 *   exp_avg_sq = fma((1 - beta2) * g, g, exp_avg_sq * beta2)
 *   max_exp_avg_sq = max(max_exp_avg_sq, exp_avg_sq)                    (amsgrad)
 *   param += -lr / (1 - beta1^step) * exp_avg / (sqrt(max_exp_avg_sq or exp_avg_sq)
 *                                                / sqrt(1 - beta2^step) + eps)
 * `step` is the already-incremented step count.  All arrays are host arrays of
 * device pointers / element counts; max_exp_avg_sq entries may be NULL without
 * amsgrad.  n <= 64 per call. */
int vp3d_adam_step(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, float* const* max_exp_avg_sq, const int64_t* numel, double lr,
                   double beta1, double beta2, double eps, double weight_decay, int64_t step, int amsgrad,
                   void* stream);

/* ---- trajectory-conditioned sequence lifters, eval mode ----
 * CoupledTransformer (common/models/CamTransformer.py:95-205) and CoupledLSTM
 * (common/models/CamLSTM.py:47-129): per frame [flat 2D | flat K.E] (:187-190 /
 * :115-121), then a transformer encoder or a stacked LSTM over a window, the last
 * step through an MLP head.  f32. */
#define VP3D_SEQ_TRANSFORMER 0
#define VP3D_SEQ_LSTM 1
#define VP3D_SEQ_MAX_HEAD 8

typedef struct vp3d_seq_cfg {
    int32_t kind;            /* VP3D_SEQ_*                                                 */
    int32_t num_joints_in, in_features, num_joints_out, out_features;
    int32_t d_model;         /* transformer d_model / LSTM hidden_size                     */
    int32_t num_layers;      /* encoder layers / LSTM cells (<= 4)                         */
    int32_t n_heads;         /* transformer only; d_model / n_heads in {16, 32, 64}        */
    int32_t dim_feedforward; /* transformer only                                           */
    int32_t n_head_layers;   /* len(head_layers)                                           */
    int32_t head_layers[VP3D_SEQ_MAX_HEAD];
    int32_t max_len;         /* rows of the positional-encoding table (5000)               */
    float eps;               /* LayerNorm / BatchNorm eps (1e-5)                           */
} vp3d_seq_cfg;

typedef struct vp3d_seq_lifter vp3d_seq_lifter;

/* Host weight arrays vp3d_seq_create expects, in state_dict order without the
 * BatchNorm num_batches_tracked counters:
 *   transformer: input_projection.{weight, bias}, positional_encoding.pe (max_len x d),
 *     pre_transformer_norm.{weight, bias}, per encoder layer self_attn.in_proj_{weight, bias},
 *     self_attn.out_proj.{weight, bias}, linear1.{weight, bias}, linear2.{weight, bias},
 *     norm1.{weight, bias}, norm2.{weight, bias}; mlp_layers Linear {weight, bias} x (heads + 1)
 *   lstm: per cell weight_ih, weight_hh, bias_ih, bias_hh; bn_lstm.{weight, bias,
 *     running_mean, running_var}; per head layer Linear {weight, bias} + BatchNorm1d
 *     {weight, bias, running_mean, running_var}; the last Linear {weight, bias}
 * Returns the count, or -1 for an invalid configuration. */
int vp3d_seq_weight_count(const vp3d_seq_cfg* cfg);
int vp3d_seq_create(const vp3d_seq_cfg* cfg, const float* const* weights, int n_weights, vp3d_seq_lifter** out);
int vp3d_seq_destroy(vp3d_seq_lifter* h);

/* forward(input_2d, input_cam) (CamTransformer.py:165-205, CamLSTM.py:104-129):
 * x2d device f32 (B, T, J_in, F), xcam device f32 (B, T, 3, 4) -> y device f32
 * (B, 1, J_out, out_features). */
int vp3d_seq_forward(vp3d_seq_lifter* h, const float* x2d, const float* xcam, int B, int T, float* y, void* stream);

/* sliding_window(inputs_2d, inputs_cam, window) (CamTransformer.py:72-92): x2d (L, J_in, F),
 * xcam (L, 3, 4) of one sequence -> y (L - window + 1, J_out, out_features), window w =
 * frames [w, w + window).  The per-frame input projection is shared by all windows; no
 * (n_windows, window, ...) copy is made. */
int vp3d_seq_sliding_window(vp3d_seq_lifter* h, const float* x2d, const float* xcam, int L, int window, float* y,
                            void* stream);

/* ---- CoupledLSTM training step (opt-in; run.py:451-487 with --use-model LSTM-Coupled) ----
 * The reference trains CoupledLSTM (common/models/CamLSTM.py:47-129) in train mode inside
 * run.py's loop (:451-487: model(batch_2d, batch_cam) :470-471, mpjpe, loss.backward(),
 * optim.Adam(amsgrad=True).step() :662): nn.LSTM with its inter-layer dropout, bn_lstm and the
 * head's BatchNorm1d on batch statistics with a running-stat update, LeakyReLU(0.01), Dropout.
 * A seq trainer runs that forward and its backward through time on the device in f32, following
 * vp3d_trainer's conventions: the parameters stay in caller-owned device memory and are passed
 * per call as a table of device pointers in vp3d_seq_weight_count order (the running statistics
 * among them, updated in place); dropout masks come from the counter hash of (seed, site,
 * element) and are regenerated in the backward, never stored.  Mask sites: 0 .. L-2 the
 * inter-layer LSTM dropouts (element (b, t, u), CamLSTM.py:77 nn.LSTM(dropout=)), then one per
 * head layer (element (b, c), CamLSTM.py:91). */
typedef struct vp3d_seq_trainer vp3d_seq_trainer;

/* kind must be VP3D_SEQ_LSTM (the transformer kind is VP3D_ERR_ARG: its training is not built);
 * hidden size 64 or 128, 1..4 cells, as vp3d_seq_create. */
int vp3d_seq_trainer_create(const vp3d_seq_cfg* cfg, vp3d_seq_trainer** out);
int vp3d_seq_trainer_destroy(vp3d_seq_trainer* t);

/* Train-mode forward (CoupledLSTM.forward in train mode, CamLSTM.py:104-129).  params: host
 * array of n_params DEVICE pointers, vp3d_seq_weight_count order.  x2d device f32
 * (B, T, J_in, F), xcam device f32 (B, T, 3, 4) -> y device f32 (B, 1, J_out, out_features).
 * dropout_p: the module's dropout (nn.LSTM's inter-layer one and the head's nn.Dropout), in
 * [0, 1) else VP3D_ERR_ARG.  momenta: one BatchNorm1d.momentum per BatchNorm (bn_lstm, then the
 * head's), host doubles.  B >= 2 (batch statistics; B = 1 is VP3D_ERR_ARG), T >= 1.  The
 * activation store (vp3d_seq_train_bytes) is allocated on first use and grown on demand; a
 * failed allocation is VP3D_ERR_OOM with a message.  Kept until the next forward. */
int vp3d_seq_train_forward(vp3d_seq_trainer* t, float* const* params, int n_params, const float* x2d,
                           const float* xcam, int B, int T, float dropout_p, const double* momenta, uint64_t seed,
                           float* y, void* stream);

/* Backward of the latest vp3d_seq_train_forward (loss.backward(), run.py:477; same params).
 * dy: device f32 like y.  grads: host array of n_params device pointers; each non-NULL
 * trainable entry is overwritten with its gradient in torch layout, NULL entries are skipped,
 * running-stat entries are ignored.  The input gradient is not formed (the inputs are data).
 * VP3D_ERR_STATE without a preceding forward (the backward consumes the stored gates: one
 * backward per forward). */
int vp3d_seq_train_backward(vp3d_seq_trainer* t, float* const* params, int n_params, const float* dy,
                            float* const* grads, void* stream);

/* Test hook, for the latest forward: which = 0 the dropout keep mask (1 = kept) of `site`,
 * which = 1 the LeakyReLU side (1 = BN output > 0; head sites only).  Sites 0 .. L-2 are the
 * inter-layer LSTM dropouts, n = B * T * H, row-major (b, t, u); sites L-1 .. are the head
 * layers, n = B * width, row-major (b, c).  out: device uint8. */
int vp3d_seq_train_mask(vp3d_seq_trainer* t, int site, int which, int64_t n, uint8_t* out, void* stream);

/* Bytes of the activation store of a (B, T) forward: per (window, step, cell) the four
 * activated gates, the cell state and the hidden state, B * T * L * 6 H * 4 (1.53 GB at
 * B = 1024, T = 243, L = 2, H = 128).  The trainer's one device allocation is larger, about 1.5
 * times that at the shape above: on top come layer 0's gate pre-activations (B * T * 4 H floats,
 * 0.51 GB there), the input rows (B * T * (J_in * F + 12) floats, 0.05 GB), with two or more
 * cells one scratch copy of a cell's dropped output rows (B * T * H floats, 0.13 GB), a zero
 * row per (window, cell) in front of c and h, 64 MB of weight-gradient partials, and the head's
 * B rows.  Host arithmetic only; -1 for an invalid configuration or non-positive B or T. */
int64_t vp3d_seq_train_bytes(const vp3d_seq_cfg* cfg, int B, int T);

/* Measurement (tools/bench_lstm_train.py), as vp3d_train_profile: synchronises; `ms` (may be
 * NULL) receives the device milliseconds, summed since the previous call, of [0] the recurrence
 * forward, [1] the backward through time, [2] the cells' weight-gradient GEMMs and bias column
 * sums, [3] the rest (weight packs, input rows and projection, the head, the dropped rows).
 * Then profiling is switched on or off.  While on, every launch group is bracketed by two
 * events that are kept until the next call of this function: switch it on for a measurement
 * pass of a few steps, not for a training run. */
int vp3d_seq_train_profile(vp3d_seq_trainer* t, int on, double* ms);

/* ---- stacked pose lifter: the ensemble MLP, eval mode ----
 * StackedPoseLifter (common/models/StackedPoseLifter.py:4-56; built at run.py:241-288, called
 * per sequence at run.py:719-720): Linear(2 J F -> layer_size), ReLU, Dropout, num_layers x
 * [Linear(layer_size -> layer_size), ReLU, Dropout], Linear(layer_size -> J F) on rows of
 * [transformer prediction | FCN prediction] (:46-49).  One kernel launch, exact f32. */
#define VP3D_STACKED_MAX_LAYERS 8
#define VP3D_STACKED_MAX_LAYER_SIZE 512
#define VP3D_STACKED_MAX_POSE 512 /* num_joints * features */

typedef struct vp3d_stacked_cfg {
    int32_t num_joints, features; /* StackedPoseLifter.py:16-17                             */
    int32_t num_layers;           /* hidden Linear(layer_size, layer_size) layers (:27-30), 0..8 */
    int32_t layer_size;           /* :20, 1..512                                            */
} vp3d_stacked_cfg;

typedef struct vp3d_stacked vp3d_stacked;

/* Host weight arrays vp3d_stacked_create expects: the state_dict order of the mlp_layers
 * ModuleList (StackedPoseLifter.py:22-34), mlp_layers.{0, 3, 6, ...}.{weight, bias}:
 * 2 * (num_layers + 2) arrays.  Returns the count, or -1 for an invalid configuration. */
int vp3d_stacked_weight_count(const vp3d_stacked_cfg* cfg);
/* Validates the configuration first (VP3D_ERR_ASSERT and a message naming the limit, before
 * any device call), then packs the weights into one device buffer in the kernel's operand order. */
int vp3d_stacked_create(const vp3d_stacked_cfg* cfg, const float* const* weights, int n_weights, vp3d_stacked** out);
/* forward(input_3d_transformer, input_3d_FCN) (StackedPoseLifter.py:37-56): y_transformer and
 * y_fcn device f32 (n_rows, J * F), contiguous -> out device f32 (n_rows, J * F).  A row's
 * result depends on that row alone (not on n_rows or its position), bit for bit. */
int vp3d_stacked_forward(vp3d_stacked* h, const float* y_transformer, const float* y_fcn, int64_t n_rows, float* out,
                         void* stream);
int vp3d_stacked_destroy(vp3d_stacked* h);

/* ---- on-device input path (common/camera.py, common/generators.py) ---- */

/* normalize_screen_coordinates (camera.py:14-18): out = X/w*2 - [1, h/w] for
 * n_points (x, y) pairs, with the reference's float64 promotion of the offset
 * reproduced exactly (quirk Q6).  Device pointers, in-place allowed. */
int vp3d_normalize_screen(const float* x, int64_t n_points, int32_t w, int32_t h, float* out,
                          void* stream);

/* normalize_screen_coordinates on float64 keypoints with a non-integral resolution (the
 * 3DPW path: keypoints stored f64, w = 2 c_x a float32 scalar, run.py:117 /
 * ThreeDPWDataset.py:87-103): out = f32(X/w*2 - [1, hw]) with the whole expression in
 * float64, i.e. the reference's float64 result rounded once when its generator casts the
 * batch (run.py:458).  hw = the value h / w takes in the caller's arithmetic (float32
 * division for float32 w, h). */
int vp3d_normalize_screen_f64(const double* x, int64_t n_points, double w, double hw, float* out,
                              void* stream);

/* image_coordinates (camera.py:21-25): out = (X + [1, h/w]) * w / 2. */
int vp3d_image_coordinates(const float* x, int64_t n_points, int32_t w, int32_t h, float* out,
                           void* stream);

/* Per-frame camera matrices K @ E_t (generators.py:115-125, :180-190).
 * intr: device f32 [fx, fy, cx, cy] per sequence (n_seq x 4); frame_seq: device
 * int32 sequence id of each frame; extr: device f64 (n_frames, 3, 4) extrinsics;
 * out: device f32 (n_frames, 12).  Evaluated in float64 like the reference's
 * float32 @ float64 numpy matmul, then rounded once to f32. */
int vp3d_camera_matrices(const float* intr, const int32_t* frame_seq, const double* extr,
                         int64_t n_frames, float* out, void* stream);

/* world_to_camera (camera.py:28-30 -> quaternion.py:10-35):
 * out = qrot(qinverse(R), X - t) for n_points 3-vectors; R (4,) and t (3,) host
 * values (one camera per call, like the reference). */
int vp3d_world_to_camera(const float* X, int64_t n_points, const float* R_host,
                         const float* t_host, float* out, void* stream);

/* Window gather with edge padding (ChunkedGenerator.pad_chunk/next_epoch,
 * generators.py:92-137; UnchunkedGenerator edge pad :193-198), fused with the
 * trajectory concat (CamTransformer.py:187-190).
 *   kps:      device f32 (n_frames, F2) normalised 2D keypoints (F2 = J*2)
 *   cams:     device f32 (n_frames, 12) camera matrices or NULL (no concat)
 *   seq_off:  device int64 first frame of each sequence; seq_len: device int32
 *   pairs:    device int32 (B, 2) = (sequence id, first output frame start_3d)
 *   out:      device f32 (B, window, F2 [+12])
 * Window b covers frames [start_3d - pad - shift, start_3d - pad - shift + window)
 * of its sequence, indices clamped to [0, len-1] ('edge' padding). */
int vp3d_gather_windows(const float* kps, int32_t f2, const float* cams, const int64_t* seq_off,
                        const int32_t* seq_len, const int32_t* pairs, int32_t B, int32_t window,
                        int32_t pad, int32_t causal_shift, float* out, void* stream);

/* project_to_2d (camera.py:37-67: H36M radial + tangential distortion) or, with
 * linear != 0, project_to_2d_linear (:69-90): X device f32 (n_cams, pts_per_cam, 3)
 * camera-space points, params device f32 (n_cams, 9) = [f(2), c(2), k(3), p(2)],
 * out device f32 (n_cams, pts_per_cam, 2).  Same float32 operation order as the
 * reference's torch code (bit-exact on the goldens). */
int vp3d_project_to_2d(const float* X, int64_t n_cams, int64_t pts_per_cam, const float* params,
                       int32_t linear, float* out, void* stream);

/* mpjpe partial sums (loss.py:11-17): acc[0] += sum ||pred - target||_2 over
 * n_points xyz triples, acc[1] += n_points.  acc: device f64[2] (caller zeroes). */
int vp3d_mpjpe_accumulate(const float* pred, const float* target, int64_t n_points, double* acc,
                          void* stream);

/* Gradient of the training loss mpjpe = mean ||pred - target|| (loss.py:11-17, run.py:478)
 * with respect to pred: grad_pred = grad_loss[0] / n_points * (pred - target) / ||pred - target||
 * per point (0 where the distance is 0).  grad_loss: device f32 scalar (the upstream
 * gradient, 1 for loss.backward()); grad_pred: device f32 like pred. */
int vp3d_mpjpe_backward(const float* pred, const float* target, int64_t n_points, const float* grad_loss,
                        float* grad_pred, void* stream);

/* Evaluation metrics of one sequence's predictions (run.py:732-750): partial sums of
 * MPJPE (loss.py:11-17), P-MPJPE (rigid alignment per frame, loss.py:29-68), N-MPJPE
 * (per-frame scale, loss.py:70-80) and MPJVE (first difference along frames,
 * loss.py:82-91) over pred / target (n_frames, n_joints, 3), float64:
 *   acc[0..3] += summed per-joint errors (MPJPE, P-MPJPE, N-MPJPE, MPJVE)
 *   acc[4] += n_frames * n_joints,  acc[5] += (n_frames - 1) * n_joints
 * acc: device f64[6] (caller zeroes).  Metric = acc[i] / acc[4] (i < 3), acc[3] / acc[5]. */
int vp3d_pose_metrics(const float* pred, const float* target, int64_t n_frames, int32_t n_joints,
                      double* acc, void* stream);

const char* vp3d_last_error(void);
int vp3d_abi_version(void);
/* SHA-256 (hex) of the sources this library was built from: every csrc/ translation unit
 * and header plus include/vp3d.h and the compiler flags (vp3d_amd/build.py source_hash).
 * The Python loader refuses a library whose hash differs from the tree beside it. */
const char* vp3d_build_hash(void);

#ifdef __cplusplus
}
#endif

#endif /* VP3D_H */
