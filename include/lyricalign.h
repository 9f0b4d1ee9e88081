/*
 * lyricalign.h -- C ABI of liblyricalign_hip.so (MI355X / gfx950 only).
 *
 * The reference (navi0105/LyricAlignment) is pure Python and has no FFI: its
 * "operator interface" for the alignment hot path is the set of Python calls
 *
 *   whisper.audio.log_mel_spectrogram(audios)        module/align_model.py:84
 *   whisper_model.embed_audio(mel)                   module/align_model.py:91,101,112,137
 *   align_rnn(embed)   (GRU -> Mish -> Linear)        module/align_model.py:35-38,107,115
 *   perform_viterbi_ctc / perform_viterbi            utils/alignment.py:121-188 / :13-71
 *   run_viterbi_core                                 utils/alignment.py:73-119
 *
 * Every entry point below names the call it replaces.  The Python packages in
 * lyricalignment_amd/ (same names and signatures as the reference's modules)
 * bind these symbols with ctypes; INTEGRATION.md shows the stub a maintainer
 * of the reference would add.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++ / torch types cross the boundary;
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - the caller owns every buffer; scratch comes from a caller-provided
 *     workspace sized by the matching *_workspace_bytes() query;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *     calls only enqueue work: on the inference path (everything the two
 *     model-level entry points la_encoder_forward / la_align_head_forward
 *     and the alignment DP call) they never synchronise, allocate or free;
 *   - return value: la_status.  Nothing throws across the boundary.
 *     Per-utterance outcomes of the DP are reported in a device `status`
 *     array with the same codes.
 *   - re-entrant.  Library-owned state, all of it mutex-guarded:
 *       (1) the optional kernel timer (la_timer_*), for bench.py only;
 *       (2) one scratch buffer per (device, stream, purpose) for two
 *           TRAINING-path calls whose scratch size depends on a run-time split
 *           decision -- float32 la_gemm / la_gemm_ex when they split K over
 *           extra workgroups (few tiles, long K: the text decoder's 80-row
 *           GEMMs) and la_colsum_f32.  Its first use on a stream calls
 *           hipMalloc (>= 1 MiB); growing it calls hipStreamSynchronize on that
 *           stream, hipFree and hipMalloc once; it lives until the process ends.
 *           LA_GEMM_NO_SPLITK=1 keeps la_gemm off it.  No 16-bit (inference)
 *           call touches it.
 */
#ifndef LYRICALIGN_H
#define LYRICALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum la_status {
    LA_OK = 0,
    LA_EINVAL = 1,       /* bad argument (shape / alignment / null pointer)            */
    LA_EINFEASIBLE = 2,  /* a label state is never visited -> reference: ValueError    */
                         /*   ("k is not in list", utils/alignment.py:183)             */
    LA_EEMPTY = 3,       /* utterance without labels -> reference: IndexError (:152)   */
    LA_EHIP = 4,         /* HIP runtime error, see la_last_error()                     */
    LA_ETIMEOUT = 5,     /* a bounded in-kernel wait gave up (persistent GRU kernel)   */
    LA_EUNSUPPORTED = 6  /* shape outside what the gfx950 kernels are built for        */
} la_status;

typedef enum la_dtype {
    LA_F32 = 0,  /* parity mode: f32 storage, f32-input MFMA (exact fmaf chains)      */
    LA_BF16 = 1, /* throughput mode: bf16 operands, f32 accumulate, f32 residual      */
    LA_F16 = 2   /* the same kernels on IEEE half operands (BASELINE configs[3]: "fp16 MFMA"); 10-bit mantissa, range
                    +-65504 -- Whisper was trained in fp16, so its activations fit                                   */
} la_dtype;

/*
 * Modifier bit on the dtype argument of la_attention / la_attention_ex / la_attention_cached and on la_encoder_weights.dtype
 * (16-bit dtypes): the q operand -- the q rows of wqkv and of bqkv -- carries head_dim^-0.5 * log2(e) instead of
 * head_dim^-0.5 (whisper/model.py MultiHeadAttention.qkv_attention scales q and k by head_dim^-0.25 each), so the scores
 * leave the matrix pipe in the exp2 domain.  With LA_BF16 the attention kernel then also starts its running maximum at 0
 * and subtracts nothing until a query needs it (la_attention.hip, FOLD): one vector instruction less per score.
 */
#define LA_Q_LOG2 0x100


typedef enum la_variant {
    LA_VARIANT_PLAIN = 0, /* perform_viterbi:      log_softmax over all V, silence = col 0          */
    LA_VARIANT_CTC = 1    /* perform_viterbi_ctc:  log_softmax over cols 1..V-2, silence = sigmoid  */
                          /*                       of the last column (naive log, clip -1000)       */
} la_variant;

/* ------------------------------------------------------------------------- */
/* library                                                                    */
/* ------------------------------------------------------------------------- */
int la_version(void);                 /* ABI version, currently 2 (la_encoder_block / la_head_weights carry the f16x2 planes) */
const char *la_last_error(void);      /* thread-local text of the last LA_EHIP / LA_EINVAL     */
int la_device_arch_ok(void);          /* 1 if the current device is gfx950                     */

/* Optional per-kernel HIP-event timer (bench.py roofline leg).  When enabled,
 * launches of the kernel family `name` ("gemm_bf16", "attention", ...) on any
 * stream are bracketed by hipEvents; la_timer_read() synchronises those events
 * and returns the summed milliseconds and the launch count since reset.      */
int la_timer_enable(const char *name);
int la_timer_disable(void);
int la_timer_read(double *total_ms, int64_t *launches);
int la_timer_reset(void);
/* Sampling: bracket every `period`-th launch of the family only (an event record is a barrier packet of its own: ~6.6 us of stream
 * idle time each between back-to-back kernels).  la_timer_read_work also returns the summed work (flops for the GEMM families:
 * 2 M N K batch) of the bracketed launches and the number of launches of the family seen since the reset. */
int la_timer_sample(int32_t period);
int la_timer_read_work(double *total_ms, int64_t *timed_launches, double *timed_work, int64_t *all_launches);

/* Library options: the few choices between SHIPPED kernel forms that a caller (or a test) may want to pin.  Each is resolved ONCE per
 * process -- on first use, from the environment variable named below -- into a plain struct that the launch paths read; no launch
 * calls getenv.  la_set_option overrides a value at run time (between launches; not synchronised with launches in flight on other
 * threads), la_get_option reads it back.  Unknown name -> LA_EINVAL.
 *   name              env                 values
 *   "gemm_tile"       LA_GEMM_TILE        0 = by shape (default) | 128 | 256 (the 256 x 128 three-stage tile) | 512 (force the 256 x 256 kernel)
 *   "gemm_loop"       LA_PP_DBG           0 = hand-placed main loop where K % 128 == 0 (default) | 99 = quadrant ping-pong loop
 *                                         everywhere (the loop of the other K; identical bits)
 *   "gemm_splitk"     LA_GEMM_NO_SPLITK   1 = float32 GEMMs with few tiles cut K over batch slots (default) | 0 = never (no library scratch)
 *   "attn_nw"         LA_ATTN_NW          0 = 256-query workgroups from 1024 positions on (default) | 4 = 128-query | 8 = 256-query
 *   "gru_nw"          LA_GRU_NW           0 = 8-wave workgroups (default) | 4 = 4-wave workgroups of the persistent recurrence
 *   "gru_fence"       LA_GRU_FENCE        0 = write-through hand-off (default) | 1 = release / acquire fences
 *   "gru_handoff"     LA_GRU_HANDOFF      0 = data-tagged 8-byte granules, no counter, from 17 clips on (default; 16-bit, 8-wave workgroups;
 *                                         float32 training sweeps: always) | 1 = the counter form everywhere (write-through stores, drain,
 *                                         barrier, counter add; poll, barrier, loads) | 2 = granules for every batch
 *   "gru_poll_delay"  LA_GRU_POLL_DELAY   0 (default) = poll at once | n = n x 64 clocks of sleep before a step's first poll of the granule hand-off
 *   "viterbi_dpp"     LA_VITERBI_NO_DPP   1 = DPP wave shifts (default) | 0 = the LDS-exchange form
 *   "head_clip_cap"   LA_HEAD_CLIP_CAP    0 = by residency (default) | n = clips per head launch set of la_align_head_forward
 *   "ln_fusion"       LA_LN_FUSION        1 = LayerNorm folded into the 16-bit encoder GEMMs where they run on the 256 x 256 kernel | 0 = never
 *   "resid_split"     LA_RESID_SPLIT      1 = the 16-bit encoder keeps its residual stream split (hi 16-bit + lo byte) | 0 = f32 stream
 *   "gru_timeout_us"  LA_GRU_TIMEOUT_US   0 = 3 s (default) | n = bound of one inter-workgroup wait of the persistent GRU kernels in microseconds (a launch
 *                                         whose workgroups are not all co-resident never completes a hand-off: the bounded wait sets timeout_flag)
 *   "gru_fault_step"  LA_GRU_FAULT_STEP   test hook, ONE launch (the launch that reads it clears it): workgroup (0, 0, 0) of the next GRU forward launch
 *                                         leaves at step n without publishing, as if it had never become resident -- the other workgroups
 *                                         time out.  0 = off (default)
 *   "x2_inference"    LA_X2_INFERENCE     1 = float32 inference (la_encoder_forward / la_align_head_forward with LA_F32 weights that carry f16x2
 *                                         planes) on the f16 matrix pipe at float32 accuracy (default) | 0 = the float32-MFMA kernels (A/B partner)
 *   "x2_small"        LA_X2_SMALL         0 = the x2_inference route only where every product fills the 256 x 256 kernel (9 clips on at d = 1024;
 *                                         default) | 1 = at every batch size: the products outside that kernel's domain run on the 128 x 128
 *                                         f16x2 kernel (la_gemm_f16x2_small) instead of the float32-MFMA kernel (needs x2_inference = 1)
 *   "gemm_epi16"      LA_GEMM_EPI16       1 = interior output tiles of the 256 x 256 kernel with a 16-bit result and no residual (plain / LayerNorm-
 *                                         consumer epilogues) run the epilogue arithmetic in the accumulator layout and cross the LDS transpose as
 *                                         16-bit values (default) | 0 = every tile crosses it as float32 (twice the staging; identical bits: A/B partner)
 *   Cache policy of the streamed stores and loads of the 16-bit encoder's hot kernels, one option per site: a modifier bit of the same
 *   instruction (where a line is kept, never what is written; identical bits under every value).  0 = the default cache policy (the
 *   default of every option but cp_epi16); 1 = nt, the streaming hint; any other value -> LA_EINVAL.  Measurements: profiles/cache_policy.txt.
 *   "cp_epi16"        LA_CP_EPI16         the 16-byte result stores of the 256 x 256 kernel's 16-bit staging (QKV, MLP-up): 1 = nt (default:
 *                                         -0.8 ms of the 40 ms bf16 step) | 0 | 2 = sc1, write-through: the line leaves the XCD's L2 with the store
 *   "cp_split_st"     LA_CP_SPLIT_ST      la_gemm_split: the interior tiles' stores of the hi and lo planes
 *   "cp_split_ld"     LA_CP_SPLIT_LD      la_gemm_split in place: the interior tiles' loads of the incoming planes
 *   "cp_gemm_a"       LA_CP_GEMM_A        the hand-placed main loop's LDS-DMA pieces of the A operand (16-bit and split-stream results); W keeps the default
 *   "cp_attn_qo"      LA_CP_ATTN_QO       16-bit attention: the Q fragment loads and the output stores
 *   "cp_attn_kv"      LA_CP_ATTN_KV       16-bit attention: the LDS-DMA pieces of the K / V tiles
 * A library built with -DLA_EXPERIMENTS (tools/build_variant.sh; la_has_experiments() == 1) additionally carries the measured-slower
 * GEMM kernel structures of rounds 2-4 and their per-launch developer switches; the shipped library has neither.  The attention
 * kernels have one form per (element type, workgroup size, LA_Q_LOG2) in every build; their timing knock-outs are compile-time masks
 * (-DLA_ATTN_KO=<mask>, -DLA_X2F_KO=<mask>: one library per mask, tools/ab_attn_knockouts.sh), never a switch read at a launch. */
int la_set_option(const char *name, int64_t value);
int la_get_option(const char *name, int64_t *value);
int la_has_experiments(void);

/* ------------------------------------------------------------------------- */
/* forced-alignment DP   (replaces utils/alignment.py:73-119 + :141-185)      */
/* ------------------------------------------------------------------------- */
/*
 * Emissions use the COMPACT layout the fused head produces:
 *   em[b][t][0]     = log-prob of silence at frame t      (reference: ls[t][0])
 *   em[b][t][1 + n] = log-prob of label n's class          (reference: lp[t][label[n]-1])
 * (equal neighbouring labels therefore carry identical columns, as they read one class column)
 * float32, strides given in elements.  labels[b][n] are class ids (only equality
 * of neighbours is used, utils/alignment.py:104); n_labels[b] = L_b, n_frames[b] = T_b.
 *
 * Scores are accumulated in float64 with the reference's comparison order and
 * tie rules; backpointers are 2-bit offsets {0,1,2}.  Outputs are INTEGER
 * frame indices: onset[b][n] = first frame in state 2n+1, offset[b][n] = last
 * such frame + 1 (the Python layer multiplies by hop_size_second exactly as
 * utils/alignment.py:185 does).  status[b] is LA_OK / LA_EINFEASIBLE / LA_EEMPTY
 * / LA_EINVAL.  Rows n >= L_b of onset/offset are set to -1.
 * Limits: max_labels <= 4095 (one lane per lattice state up to 1024 states; beyond that 1024 threads sweep 2 / 4 / 8
 * consecutive states each, backpointers in `workspace`); LA_EUNSUPPORTED above -- the reference's numba loop has no limit.
 * `workspace` (8-byte aligned) is needed when la_viterbi_workspace_bytes() > 0: long utterances or > 511 labels.
 */
int la_viterbi_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_viterbi_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                     const int32_t *labels, int32_t labels_stride,
                     const int32_t *n_labels, const int32_t *n_frames,
                     int32_t batch, int32_t max_frames, int32_t max_labels,
                     int32_t *onset, int32_t *offset, int32_t out_stride,
                     double *final_score, int32_t *status,
                     void *workspace, size_t workspace_bytes, void *stream);

/*
 * run_viterbi_core(dp, bt, lp, ls, label) (utils/alignment.py:73-119) for ONE utterance, for callers
 * that want the full matrices: row 0 of dp [T][S] (float64, S = 2L+1) is READ as the caller initialised
 * it (the reference does the same, :144-152); rows >= 1 of dp and of bt [T][S] (int64 predecessor state)
 * are written.  em is the compact emission layout of that utterance ([T][>= L+1]).  n_labels / n_frames
 * are 1-element device arrays holding the same L and T as the host arguments; scratch_i32 has 2L+1
 * elements, scratch_f64 one.
 */
int la_viterbi_core(const float *em, int64_t em_row_stride, const int32_t *labels, int32_t n_labels_host,
                    int32_t n_frames_host, const int32_t *n_labels, const int32_t *n_frames,
                    double *dp, long long *bt, int32_t *scratch_i32, double *scratch_f64,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same DP on a lattice with OPTIONAL label spans (no counterpart in the reference, where every label must occupy at
 * least one frame): lyric sheets whose lines are not all sung.  Every argument of la_viterbi_batch in the same order, then
 * skip_from [batch][skip_stride] int32 (device, skip_stride >= max_labels + 1; entries 0 .. L_b of row b are read) and
 * skip_penalty >= 0 (float64).  skip_from[b][n] = a with 0 <= a < n declares labels a .. n-1 an optional span: a path may
 * pass from before label a to position n without visiting them.  Any other value (-1 by convention) means "no span ends
 * at n" and is never used as an index; one span per end position; n = L_b is a span at the end of the lyrics.  The two
 * states at position n -- 2n (the silence before label n, the final silence when n = L_b) and 2n+1 (label n, n < L_b) --
 * get two more predecessors: J = 2a, the silence before the span (always), and J-1 = 2a-1, the label before it (a >= 1;
 * into 2n+1 only if labels[n] != labels[a-1], the equal-neighbour rule).  Per state and frame: the existing rule picks
 * (best, source) among k, k-1, k-2; then dp[J] - skip_penalty replaces it if STRICTLY greater, then dp[J-1] - skip_penalty
 * likewise; the emission is added last.  Start states and termination are la_viterbi_batch's, so a skipped span at either
 * end of the lyrics costs one frame of the silence state there, and two adjacent spans skipped together one frame of the
 * silence between them.  All float64 adds and subtracts in this order: bit-reproducible; with every entry -1 the outputs
 * are la_viterbi_batch's bit for bit.
 * Outputs as la_viterbi_batch; labels inside a span whose jump the best path took get onset = offset = -1 with status
 * LA_OK; LA_EINFEASIBLE only if a label is unvisited and not inside a taken jump.
 * Limit: max_labels <= 511 (one lane per lattice state), LA_EUNSUPPORTED above.  Backpointers are three 64-bit masks per
 * wave per frame: `workspace` (8-byte aligned) is needed when la_viterbi_spans_workspace_bytes() > 0 (batch * max_frames *
 * waves * 24 bytes, once the masks no longer fit in LDS).  Argument errors (a negative or NaN skip_penalty included) are
 * answered on the host before anything is enqueued; never synchronises, allocates or frees.  Option viterbi_dpp = 0 pins
 * the LDS-exchange form for lattices of at most 64 states, as for la_viterbi_batch.
 */
int la_viterbi_spans_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_viterbi_spans_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                           const int32_t *labels, int32_t labels_stride,
                           const int32_t *n_labels, const int32_t *n_frames,
                           int32_t batch, int32_t max_frames, int32_t max_labels,
                           int32_t *onset, int32_t *offset, int32_t out_stride,
                           double *final_score, int32_t *status,
                           const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                           void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same DP with a FRAME WINDOW per lattice state (no counterpart in the reference): what the caller knows about time -- the
 * line start times of an LRC sheet, a boundary corrected by hand -- narrows the lattice.  Every argument of
 * la_viterbi_spans_batch up to skip_penalty in the same order (skip_from may be NULL: no span anywhere), then win_lo / win_hi
 * [batch][win_stride] int32 (device, win_stride >= 2 * max_labels + 1; entries 0 .. 2 L_b of row b are read).  State s of clip
 * b (0 = leading silence, 2n+1 = label n, 2n+2 = the silence after it) may hold the path at frame t only if
 * win_lo[b][s] <= t < win_hi[b][s]; any pair of int32 values is legal, lo >= hi closes the state, nothing is validated on the
 * device.  dp[t][s] is computed by la_viterbi_spans_batch's rule (comparison order, tie rules, span arcs, emission added last)
 * and then set to float64 -inf when the cell lies outside its window; row 0 likewise.  Termination is unchanged.  If the winning
 * final score is -inf no path lies inside the windows: status LA_EINFEASIBLE, final_score -inf, every onset and offset -1.
 * Otherwise backtrace, outputs and status are la_viterbi_spans_batch's (as for a clip too short for its labels, the -1e7
 * initial value of the states >= 2 at frame 0 can carry a finite score to the end when only later frames are closed: the
 * path then misses a label and the status is LA_EINFEASIBLE).  With every window [0, T_b) the outputs are
 * la_viterbi_batch's (no spans) and la_viterbi_spans_batch's (spans) bit for bit.
 * Windows are per STATE, not per label, because a bound on a label's onset from above is a bound on the states before it: a
 * window on the label alone lets the silence before it stretch past the bound.
 * Limit, workspace (la_viterbi_windows_workspace_bytes() = la_viterbi_spans_workspace_bytes()) and option viterbi_dpp as
 * la_viterbi_spans_batch.  Argument errors (null win_lo / win_hi, a win_stride below 2 * max_labels + 1, a negative or NaN
 * skip_penalty, more than 511 labels: LA_EUNSUPPORTED) are answered on the host before anything is enqueued; never
 * synchronises, allocates or frees.
 */
int la_viterbi_windows_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_viterbi_windows_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                             const int32_t *labels, int32_t labels_stride,
                             const int32_t *n_labels, const int32_t *n_frames,
                             int32_t batch, int32_t max_frames, int32_t max_labels,
                             int32_t *onset, int32_t *offset, int32_t out_stride,
                             double *final_score, int32_t *status,
                             const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                             const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * The general DP entry: the lattice of la_viterbi_windows_batch for up to 4095 labels (whole songs against whole lyric sheets).
 * Every argument of la_viterbi_windows_batch in the same order.  skip_from may be NULL (no span anywhere); win_lo / win_hi may BOTH be
 * NULL (no windows; one of them null and the other not is LA_EINVAL).  The lattice, the comparison order, the tie rules, the float64
 * arithmetic and the window gate are la_viterbi_windows_batch's; outputs and status likewise.
 * max_labels <= 511: the call runs the kernels of the matching entry and its outputs are that entry's bit for bit --
 * la_viterbi_windows_batch with windows, la_viterbi_spans_batch with spans and no windows, la_viterbi_batch with neither.
 * 512 <= max_labels <= 4095: 1024 threads sweep 2 / 4 / 8 consecutive states each, as in la_viterbi_batch (which is what runs when
 * neither spans nor windows are given); with spans or windows every thread exchanges all its states through the LDS row where the
 * clip has a span, and the backpointers are three 64-bit masks per (frame, state slot, wave).  LA_EUNSUPPORTED above 4095.
 * la_viterbi_lattice_workspace_bytes(): la_viterbi_spans_workspace_bytes()' answer up to 511 labels, above that
 * batch * max_frames * R * 16 * 3 * 8 bytes with R = 2, 4, 8 the states per thread (2 * max_labels + 1 <= 1024 R); `workspace` is
 * 8-byte aligned.  Argument errors (la_viterbi_windows_batch's, for the pointers that are present: a skip_stride below
 * max_labels + 1 with a skip_from, a win_stride below 2 * max_labels + 1 with windows, a negative or NaN skip_penalty) are answered
 * on the host before anything is enqueued; never synchronises, allocates or frees.
 * The posterior sweeps (la_alignment_posteriors*) and la_anchored_alignment_loss keep their limit of 511 labels.
 */
int la_viterbi_lattice_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_viterbi_lattice_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                             const int32_t *labels, int32_t labels_stride,
                             const int32_t *n_labels, const int32_t *n_frames,
                             int32_t batch, int32_t max_frames, int32_t max_labels,
                             int32_t *onset, int32_t *offset, int32_t out_stride,
                             double *final_score, int32_t *status,
                             const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                             const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * Repeated lyric lines: the DP of la_viterbi_lattice_batch on the lattice with REPEATABLE label spans -- a chorus printed once and sung
 * twice.  la_viterbi_lattice_batch's arguments through win_stride, then
 *   repeat_from [batch][repeat_stride] (repeat_stride >= max_labels; entries 0 .. L_b - 1 of row b are read; may be NULL): repeat_from[a]
 *       = e with a < e <= L_b declares labels a .. e-1 repeatable: having finished label e-1 the path may return to label a.  Any other
 *       value (-1 by convention) = no repeat span starts at a; it is never used as an index.  One repeat span per start position; spans
 *       may nest or overlap.
 *   repeat_penalty (>= 0, not NaN): charged per taken repeat arc.  There is no bound on the number of repetitions but this.
 *   path [batch][path_stride] (path_stride >= max_frames; may be NULL): the lattice state at every frame t < T_b; -1 for t >= T_b and
 *       for a clip without a backtrace (LA_EEMPTY, LA_EINVAL, no path inside the windows).
 * The only new target is the odd state 2a+1.  It gets two more predecessors, both from the previous frame: K = 2e, the silence after
 * the span (always), and K-1 = 2e-1, label e-1, only if labels[a] != labels[e-1] (the equal-neighbour rule: a one-label span returns
 * through the silence alone).  The DP is frame-synchronous, so an arc to the left makes no cycle.  Per cell: the existing rule, then
 * the optional span's J and J-1, then dp[K] - repeat_penalty and dp[K-1] - repeat_penalty, each replacing the winner only if STRICTLY
 * greater; the emission is added last and the window gate applies as in la_viterbi_windows_batch.  Start states and termination are
 * unchanged; everything is float64 in this order, so results are reproducible to the bit.
 * onset / offset are those of a label's FIRST visit in time (a visit = a maximal run of frames in one odd state; `path` holds them
 * all).  A label inside a taken skip jump on one pass and visited on another has its visit's onset, not -1.  status is LA_OK iff
 * every label is visited at least once or lies inside a skip jump the path took, else LA_EINFEASIBLE.
 * With repeat_from NULL or all -1, onset, offset, final_score and status equal la_viterbi_lattice_batch's bit for bit.
 * Up to 4095 labels (LA_EUNSUPPORTED above).  la_viterbi_repeats_workspace_bytes() = la_viterbi_lattice_workspace_bytes(); the
 * backpointers are three 64-bit masks whatever is given.  Argument errors (la_viterbi_lattice_batch's, a repeat_stride below max_labels
 * with a repeat_from, a path_stride below max_frames with a path, a negative or NaN repeat_penalty) are answered on the host before
 * anything is enqueued; never synchronises, allocates or frees.  The sum-product sweep of this lattice is la_alignment_posteriors_repeats
 * (up to 511 labels); the four older posterior entries and the training loss do not know this lattice.
 */
int la_viterbi_repeats_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_viterbi_repeats_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                             const int32_t *labels, int32_t labels_stride,
                             const int32_t *n_labels, const int32_t *n_frames,
                             int32_t batch, int32_t max_frames, int32_t max_labels,
                             int32_t *onset, int32_t *offset, int32_t out_stride,
                             double *final_score, int32_t *status,
                             const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                             const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                             const int32_t *repeat_from, int32_t repeat_stride, double repeat_penalty,
                             int32_t *path, int32_t path_stride,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * Free line order: the DP on the lattice of an UNMARKED lyric sheet -- the caller gives the line breaks and nothing else, and the lines
 * may be sung in any order, any number of times, or not at all (a sheet prints V1 C V2 B once each; the song sings V1 C V2 C B C).
 * la_viterbi_batch's arguments through status, then
 *   line_start [batch][line_stride] (line_stride >= max_labels; entries 0 .. L_b - 1 of row b are read): nonzero = label n begins a
 *       line.  Entry 0 must be nonzero: a clip where it is zero gets LA_EINVAL, its batch mates are unaffected.  Line m covers the
 *       labels from its start up to the next start, or up to L_b; the line ENDS e are the starts other than 0, and L_b.
 *   line_jump_penalty (>= 0, not NaN; +inf allowed): charged per jump, per free start and per free end.
 *   path [batch][path_stride] (path_stride >= max_frames; may be NULL): as la_viterbi_repeats_batch.
 * Jump sources: state 0 and, for every line end e, the states 2e-1 (the line's last label) and 2e (the silence after it); a source's
 * class is labels[s >> 1] for an odd state and "none" for a silence.  Jump targets: the odd state 2a+1 of every line start a, from any
 * source of the previous frame whose class differs from labels[a] (the equal-neighbour rule; a silence always differs).  Among the
 * allowed sources the largest dp[t-1][s] wins (the raw value), the smallest state among equals, and the jump is taken only if
 * dp[t-1][s] - line_jump_penalty is STRICTLY greater than the existing rule's winner; the emission is added last.
 * Free start: row 0 is la_viterbi_batch's, and every line start a other than 0 gets em[0][1+a] - line_jump_penalty.  Free end: the
 * choice between S-1 and S-2 first; then the best source other than 0, S-1 and S-2 (largest value, smallest state) replaces it only if
 * its value minus the penalty is strictly greater.  Float64 adds and subtracts in this order: reproducible to the bit, alone or in a
 * batch.  The kernel does O(S) work per frame whatever the number of lines (csrc/la_line_order.hip, DESIGN.md "Free line order").
 * onset / offset are those of a label's FIRST visit in time, -1 / -1 for a label never visited; status is LA_OK even then (lines may
 * be left out), LA_EEMPTY / LA_EINVAL as in la_viterbi_batch.  With line_jump_penalty = +inf the outputs are la_viterbi_batch's bit for
 * bit; with a single line they are la_viterbi_repeats_batch's with repeat_from[0] = L_b and the same penalty, up to the order of a tie.
 * Up to 4095 labels (LA_EUNSUPPORTED above).  The workspace (always needed, 8-byte aligned) holds two 64-bit backpointer masks per
 * (frame, 64 states) and two int32 per frame.  Argument errors are answered on the host before anything is enqueued; never
 * synchronises, allocates or frees.  The posteriors of this lattice are la_alignment_posteriors_lines (below); no training loss exists
 * on it.
 */
int la_viterbi_lines_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_viterbi_lines_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                           const int32_t *labels, int32_t labels_stride,
                           const int32_t *n_labels, const int32_t *n_frames,
                           int32_t batch, int32_t max_frames, int32_t max_labels,
                           int32_t *onset, int32_t *offset, int32_t out_stride,
                           double *final_score, int32_t *status,
                           const int32_t *line_start, int32_t line_stride, double line_jump_penalty,
                           int32_t *path, int32_t path_stride,
                           void *workspace, size_t workspace_bytes, void *stream);

/*
 * Minimum character duration: the DP on the PLAIN lattice with a floor, in frames, under every visit to a label (a sung syllable is never
 * one 20 ms frame long; la_viterbi_batch lets it be).  la_viterbi_lines_batch's arguments with
 *   min_frames [batch][min_frames_stride] (min_frames_stride >= max_labels; entries 0 .. L_b - 1 of row b are read): D_n, the least
 *       number of frames label n lasts, 1 .. max_min_frames.  A clip with an entry outside that range gets LA_EINVAL, its batch mates
 *       are unaffected.
 *   max_min_frames (1 .. 8, i.e. up to 160 ms at the model's hop): the bound on the floors of this call; it picks the depth of the
 *       kernel's chain (2, 4 or 8) and nothing else.
 * in the place of line_start, line_stride, line_jump_penalty.  Label n carries D_n - 1 "young" values y_1 .. y_{D-1} (in its j-th frame)
 * and one "mature" value m (has lasted at least D_n frames); only m is visible to the label's successors.
 *   Row 0: dp[0][0] = em[0][0]; label 0 has m = em[0][1] if D_0 == 1, else y_1 = em[0][1] and m = -1e7; every other value is -1e7.
 *   Row t reads row t-1 only (out_n = m_n[t-1], sil_i = state 2i, can_skip = n >= 1 && labels[n] != labels[n-1]): state 0 stays; the
 *   silence 2n+2 stays iff sil_{n+1}[t-1] > out_n (strict), else it comes from out_n; a label with D_n == 1 follows la_viterbi_batch's
 *   rule on (m_n[t-1], sil_n[t-1], out_{n-1}); a label with D_n >= 2 is ENTERED from out_{n-1} if can_skip and out_{n-1} >= sil_n[t-1],
 *   else from sil_n[t-1] (no stay candidate): y_1[t] = entry + em, y_j[t] = y_{j-1}[t-1] + em, and m[t] = (m[t-1] > y_{D-1}[t-1] ?
 *   m[t-1] : y_{D-1}[t-1]) + em.  The emission is added last; everything is float64.
 *   Termination: the backtrace starts at 2L iff sil_L[T-1] > m_{L-1}[T-1] (strict), else at the last label's mature value -- the last
 *   visit reaches its floor too; final_score is that value.  A mature cell that graduated at frame t puts its label on frames
 *   t-D_n+1 .. t and the backtrace goes on from that first frame's entry.
 * status: LA_OK iff the backtrace arrives at frame 0 in state 0 or in the first frame of label 0; otherwise LA_EINFEASIBLE (the clip is
 * shorter than its floors ask for), every onset / offset / path entry of the clip is -1 and final_score is still written.  LA_EEMPTY /
 * LA_EINVAL as in la_viterbi_batch.  With every floor 1 onset, offset, final_score and status are la_viterbi_batch's bit for bit (on an
 * infeasible clip status and score; the plain entry leaves partial rows there).  onset / offset / path as la_viterbi_lines_batch; every
 * reported label has offset - onset >= D_n.  Up to 4095 labels (LA_EUNSUPPORTED above).  The workspace (always needed, 8-byte aligned)
 * holds three 64-bit backpointer masks per (frame, 64 states).  Argument errors -- null pointers, strides below max_labels,
 * max_min_frames outside 1 .. 8, a workspace too small or misaligned -- are answered on the host before anything is enqueued; batch == 0
 * is LA_OK; never synchronises, allocates or frees.  Reproducible to the bit, alone or in a batch.  No posteriors and no training loss
 * exist on this lattice, and the span, window, repeat and line-order lattices have no floor (csrc/la_min_duration.hip, DESIGN.md
 * "Minimum duration").  No floor has been tuned on real singing.
 */
int la_viterbi_min_duration_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, int32_t max_min_frames, size_t *bytes);

int la_viterbi_min_duration_batch(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                  const int32_t *labels, int32_t labels_stride,
                                  const int32_t *n_labels, const int32_t *n_frames,
                                  int32_t batch, int32_t max_frames, int32_t max_labels,
                                  int32_t *onset, int32_t *offset, int32_t out_stride,
                                  double *final_score, int32_t *status,
                                  const int32_t *min_frames, int32_t min_frames_stride, int32_t max_min_frames,
                                  int32_t *path, int32_t path_stride,
                                  void *workspace, size_t workspace_bytes, void *stream);

/*
 * Per-character alignment confidence: forward-backward (sum-product) on the SAME lattice (no counterpart in the
 * reference, whose utils/alignment.py is max-product only).  Start states 0 and 1, end states S-1 and S-2, transitions
 * into k from k, k-1 and (odd k >= 3, differing neighbour labels) k-2; a path weighs exp(sum_t e_t(path_t)); unreachable
 * cells weigh zero.  With alpha / beta the forward / backward log-sums (both including e_t(k)) and
 * log_z = logsumexp(alpha_{T-1}(S-1), alpha_{T-1}(S-2)):
 *   gamma_t(k) = exp(alpha_t(k) + beta_t(k) - e_t(k) - log_z)          P(the path is in state k at frame t)
 *   entry_t(n) = P(frame t is the FIRST frame of label n),  exit_t(n) = P(frame t is its LAST frame)
 * em, labels, n_labels, n_frames as la_viterbi_batch; onset / offset are la_viterbi_batch's outputs for the same
 * emissions (device, row pitch out_stride); boundary_window = w >= 0 frames.  Outputs ([batch][out_stride] float32):
 *   occupancy[b][n]   = mean over t in [onset, offset) of gamma_t(2n+1): the share of the model's belief that the
 *                       reported segment is this character
 *   onset_prob[b][n]  = sum of entry_t(n) over |t - onset| <= w;  offset_prob[b][n] = sum of exit_t(n) over
 *                       |t - (offset - 1)| <= w: probability that the boundary lies within w frames of the reported one
 *   log_z[b] (float64): final_score[b] - log_z[b] <= 0 is the log-posterior of the reported path
 *   gamma_out (optional, NULL = none) [batch][max_frames][>= 2 max_labels + 1] float32, strides in elements:
 *                       gamma_t(k), zero outside T_b / S_b
 *   status[b] = LA_OK; LA_EEMPTY (no labels); LA_EINFEASIBLE (log_z = -inf: no path, T_b too short for the labels);
 *               LA_EINVAL (T_b / L_b outside max_frames / max_labels).  Rows of failed utterances, rows n >= L_b and
 *               labels with onset < 0 are written as 0; log_z of a failed utterance is 0 (-inf when infeasible).
 * These are posteriors UNDER THE MODEL, comparable between utterances; they are not measured accuracies.
 * Scores are float64; a step's log-sum-exp takes its maximum in float64 and its correction (in [0, ln 3]) in float32:
 * every probability and log_z within 8 T 2^-23 absolute of a float64 evaluation (measured: DESIGN.md).
 * `workspace` (8-byte aligned, always needed) holds the alpha rows: batch * max_frames * S_pad * 8 bytes, S_pad = 64 *
 * the smallest power of two of waves that holds 2 max_labels + 1 states (25 MB for 32 clips of 1500 frames and up to
 * 31 labels).  Limit: max_labels <= 511 (one lane per lattice state, 1024 states per workgroup; the CTC loss's limit),
 * LA_EUNSUPPORTED above.  Argument errors are answered on the host before anything is enqueued.  Option viterbi_dpp = 0
 * also pins this kernel's LDS-exchange form for lattices of at most 64 states.
 */
int la_alignment_posteriors_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_alignment_posteriors(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                            const int32_t *labels, int32_t labels_stride,
                            const int32_t *n_labels, const int32_t *n_frames,
                            int32_t batch, int32_t max_frames, int32_t max_labels,
                            const int32_t *onset, const int32_t *offset, int32_t out_stride,
                            int32_t boundary_window,
                            float *occupancy, float *onset_prob, float *offset_prob,
                            double *log_z, int32_t *status,
                            float *gamma_out, int64_t gamma_batch_stride, int64_t gamma_row_stride,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * Confidence on the lattice with OPTIONAL SPANS: the sum-product sweep of la_viterbi_spans_batch's lattice (same skip_from /
 * skip_penalty; no counterpart in the reference).  S = 2L+1 states, start states 0 and 1, end states S-1 and S-2; into state
 * s from s, s-1 and (odd s >= 3, differing neighbour labels) s-2; and, for skip_from[n] = a with 0 <= a < n, into the two
 * states at position n (2n, and 2n+1 when n < L) also from J = 2a and from J-1 (a >= 1; into the odd target only if
 * labels[n] != labels[a-1]).  A jump arc multiplies the path weight by exp(-skip_penalty).  No arc arises twice from these
 * rules, so every path counts once.  With alpha / beta including e_t(k) as above:
 *   log_z, gamma_t(k), entry_t(n), exit_t(n), occupancy, onset_prob, offset_prob: as la_alignment_posteriors, the jump arcs
 *                       being part of the incoming sums (entry) and of the outgoing sums (exit)
 *   present_prob[b][n]   = sum over t of entry_t(n): probability that label n is on the path at all ("was it sung")
 *   span_skip_prob[b][n] = sum over t >= 1, destination in {2n, 2n+1} and source in {J, J-1 where allowed} of
 *                          exp(alpha_{t-1}(source) - skip_penalty + beta_t(destination) - log_z): probability that the path
 *                          takes the jump of the span that ENDS at position n; 0 where no span ends
 * A path is monotone and leaves label n out only by one jump that covers it: for every label,
 *   present_prob[n] + sum over spans (a, e) with a <= n < e of span_skip_prob[e] = 1.
 * onset / offset are la_viterbi_spans_batch's outputs for the same skip_from and skip_penalty: labels with onset -1 (inside a
 * taken jump) get occupancy = onset_prob = offset_prob = 0, their present_prob is still written.  present_prob
 * [batch][out_stride], span_skip_prob [batch][skip_stride] (entries 0 .. max_labels of a row are written), float32.  A clip
 * without any span gets present_prob = 1 for its labels (identically true there, not summed) and its other outputs are
 * la_alignment_posteriors' bit for bit.  Statuses, zeroing of failed rows (present_prob and span_skip_prob rows too) and of
 * rows n >= L_b, gamma_out, the workspace (same size formula) and the limit max_labels <= 511 as la_alignment_posteriors.
 * The jump terms are folded in float64, in a fixed order (no atomics: a clip's result does not depend on its batch mates):
 * the error bound 8 T 2^-23 holds unchanged.  Argument errors (a negative or NaN skip_penalty, skip_stride < max_labels + 1
 * included) are answered on the host before anything is enqueued.
 */
int la_alignment_posteriors_spans_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_alignment_posteriors_spans(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                  const int32_t *labels, int32_t labels_stride,
                                  const int32_t *n_labels, const int32_t *n_frames,
                                  int32_t batch, int32_t max_frames, int32_t max_labels,
                                  const int32_t *onset, const int32_t *offset, int32_t out_stride,
                                  int32_t boundary_window,
                                  const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                                  float *occupancy, float *onset_prob, float *offset_prob, float *present_prob,
                                  float *span_skip_prob,
                                  double *log_z, int32_t *status,
                                  float *gamma_out, int64_t gamma_batch_stride, int64_t gamma_row_stride,
                                  void *workspace, size_t workspace_bytes, void *stream);

/*
 * Confidence GIVEN what the caller knows about time: the sum-product sweep of la_viterbi_windows_batch's lattice (no counterpart
 * in the reference).  Every argument of la_alignment_posteriors_spans up to skip_penalty in the same order (skip_from may be
 * NULL: no span anywhere; skip_stride is also the row pitch of span_skip_prob and must be >= max_labels + 1 either way), then
 * win_lo / win_hi [batch][win_stride] int32 as la_viterbi_windows_batch (device, win_stride >= 2 * max_labels + 1; entries
 * 0 .. 2 L_b of row b are read; any pair of int32 values is legal, lo >= hi closes the state), then the outputs and the
 * workspace of la_alignment_posteriors_spans, unchanged.  A cell (t, s) weighs zero unless win_lo[b][s] <= t < win_hi[b][s]:
 * the sweep runs over exactly the paths la_viterbi_windows_batch maximises over, and log_z is the log-sum over THOSE paths, so
 *   gamma, occupancy, onset_prob, offset_prob, present_prob, span_skip_prob are posteriors given the windows (gamma_t(s) is
 *   exactly 0 outside the window of s; rows of gamma still sum to 1; the coverage identity of la_alignment_posteriors_spans
 *   holds), and final_score[b] of la_viterbi_windows_batch - log_z[b] <= 0 is the log-posterior of its path given the windows;
 *   log_z[b] - (log_z[b] of la_alignment_posteriors_spans / la_alignment_posteriors on the same emissions) <= 0 is the
 *   log-probability the unanchored model gives to "the path lies inside the windows": near 0 when the windows agree with the
 *   audio, strongly negative when one of them fights it.
 * onset / offset are la_viterbi_windows_batch's outputs for the same windows, skip_from and skip_penalty.  No path inside the
 * windows: status LA_EINFEASIBLE, log_z -inf, every output row and gamma 0 (as for a clip too short for its labels).  Other
 * statuses, zeroing, gamma_out, the limit max_labels <= 511, option viterbi_dpp and the error bound 8 T 2^-23 as
 * la_alignment_posteriors_spans (a closed cell is exactly -inf and adds no rounding); a clip without a span gets
 * present_prob = 1 for its labels and span_skip_prob = 0.  With every window [0, T_b) the outputs are
 * la_alignment_posteriors_spans' bit for bit (with a NULL or all -1 skip_from the shared ones are la_alignment_posteriors').
 * la_alignment_posteriors_windows_workspace_bytes() = la_alignment_posteriors_spans_workspace_bytes().  Argument errors (null
 * win_lo / win_hi, a win_stride below 2 * max_labels + 1, la_alignment_posteriors_spans' other checks; more than 511 labels:
 * LA_EUNSUPPORTED) are answered on the host before anything is enqueued; never synchronises, allocates or frees.
 */
int la_alignment_posteriors_windows_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_alignment_posteriors_windows(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                    const int32_t *labels, int32_t labels_stride,
                                    const int32_t *n_labels, const int32_t *n_frames,
                                    int32_t batch, int32_t max_frames, int32_t max_labels,
                                    const int32_t *onset, const int32_t *offset, int32_t out_stride,
                                    int32_t boundary_window,
                                    const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                                    const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                    float *occupancy, float *onset_prob, float *offset_prob, float *present_prob,
                                    float *span_skip_prob,
                                    double *log_z, int32_t *status,
                                    float *gamma_out, int64_t gamma_batch_stride, int64_t gamma_row_stride,
                                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Whole-song confidence: the sum-product sweep on any face of the lattice at any size up to 4095 labels -- the posteriors'
 * counterpart of la_viterbi_lattice_batch.  The arguments are la_alignment_posteriors_windows' in the same order, with skip_from
 * and the pair win_lo / win_hi each optional (NULL): both NULL sweeps the plain lattice, skip_from alone the optional-span lattice,
 * windows (with or without skip_from) the windowed one.  win_lo without win_hi (or the reverse) is LA_EINVAL.  present_prob and
 * span_skip_prob are always written (skip_stride is the row pitch of span_skip_prob and must be >= max_labels + 1 whatever the
 * face): on a lattice without a span present_prob is 1 on the labels n < L_b of an LA_OK clip and 0 elsewhere, span_skip_prob is 0.
 *   max_labels <= 511: the call IS the matching entry above (la_alignment_posteriors_windows / _spans; with nothing given
 *     la_alignment_posteriors for the five common outputs), bit for bit, and the workspace query returns that entry's answer.
 *   512 <= max_labels <= 4095: one workgroup of 1024 threads per clip, R = 2 / 4 / 8 consecutive states per thread for up to
 *     2048 / 4096 / 8192 states.  Every cell is computed by the same expression sequence as in the entries above, so the outputs
 *     of a clip do not depend on max_labels, on its batch mates or on which of the two forms ran it, and the bound 8 T 2^-23
 *     carries over.  The workspace is batch * max_frames * 1024 R * 8 bytes of alpha rows plus batch * 1024 R * 28 bytes (the
 *     sparse per-label sums and the jump arcs by source): one clip of 12000 frames takes 197 MB at 800 labels and 786 MB at
 *     2500 .. 4095.  It must be 16-byte aligned.
 *   max_labels > 4095: LA_EUNSUPPORTED.
 * onset / offset are la_viterbi_lattice_batch's outputs for the same lattice.  Statuses, zeroing, gamma_out and its strides as in
 * la_alignment_posteriors_windows.  Every argument error is answered on the host under this entry's name before anything is
 * enqueued; never synchronises, allocates or frees.
 */
int la_alignment_posteriors_lattice_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_alignment_posteriors_lattice(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                    const int32_t *labels, int32_t labels_stride,
                                    const int32_t *n_labels, const int32_t *n_frames,
                                    int32_t batch, int32_t max_frames, int32_t max_labels,
                                    const int32_t *onset, const int32_t *offset, int32_t out_stride,
                                    int32_t boundary_window,
                                    const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                                    const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                    float *occupancy, float *onset_prob, float *offset_prob, float *present_prob,
                                    float *span_skip_prob,
                                    double *log_z, int32_t *status,
                                    float *gamma_out, int64_t gamma_batch_stride, int64_t gamma_row_stride,
                                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Confidence for repeated lyric lines: the sum-product sweep on the lattice of la_viterbi_repeats_batch.  The arguments are
 * la_alignment_posteriors_lattice's through win_stride (skip_from and the pair win_lo / win_hi each optional), then
 *   repeat_from, repeat_stride, repeat_penalty: as la_viterbi_repeats_batch (repeat_from may be NULL: no repeat span);
 *   path [batch][path_stride] (path_stride >= max_frames; may be NULL): la_viterbi_repeats_batch's `path` for the same lattice;
 * then the outputs, with `visits` where present_prob stood, and two more:
 *   repeat_count [batch][out_stride], path_prob [batch][path_stride] (may be NULL; needs path).
 * onset / offset are la_viterbi_repeats_batch's outputs for the same lattice: a label's FIRST visit.
 * A path may visit a label more than once on this lattice, so some sums that are probabilities on the other lattices are EXPECTED
 * COUNTS here and can exceed 1 (values above 2 occur with soft emissions).  No output is clamped.
 *   gamma_t(k), log_z, occupancy: unchanged in meaning (rows of gamma sum to 1; occupancy is about the first visit's segment).
 *   entry_t(n): the probability that A visit of label n begins at frame t; exit_t(n): that a visit ends there.  The repeat arcs
 *       K -> 2a+1 and K-1 -> 2a+1 count as entries of label a and as exits of their source.
 *   visits[n] = sum_t entry_t(n): the expected number of visits of label n.  Equal to present_prob where no repeat span exists.
 *   onset_prob / offset_prob[n]: the expected number of visits that begin / end within boundary_window frames of the reported
 *       boundary; probabilities whenever two visits of the label cannot begin within 2 boundary_window + 1 frames of each other.
 *   repeat_count[a]: the expected number of times the path takes a repeat arc of the span that starts at a (0 where none starts):
 *       sum over t >= 1 and the sources K and (where allowed) K-1 of exp(alpha_{t-1}(src) - repeat_penalty + beta_t(2a+1) - log_z).
 *   span_skip_prob[n]: its formula unchanged; an expected count where a repeat span covers the optional span (a skip per pass).
 *   path_prob[b][t] = gamma_t(path[b][t]), 0 for t >= T_b, for a path value that names no state and for failed clips: the
 *       occupancy of every visit, not only the first, is the mean of path_prob over the visit's frames.
 * For every label n:  visits[n] + sum over optional spans (a', e') with a' <= n < e' of span_skip_prob[e']
 *                     = 1 + sum over repeat spans (a, e) with a <= n < e of repeat_count[a].
 * Backward a source folds the arcs that leave it in one fixed order (skip targets ascending, then repeat targets ascending), no
 * atomics: a clip's numbers do not depend on its batch mates and two calls agree to the bit.  With repeat_from NULL or all -1,
 * occupancy, onset_prob, offset_prob, span_skip_prob, log_z, status and gamma_out equal la_alignment_posteriors_lattice's bit for
 * bit, visits equals its present_prob and repeat_count is 0.
 * Up to 511 labels (LA_EUNSUPPORTED above); the workspace is la_alignment_posteriors_windows' size.  Statuses and the zeroing of
 * failed rows as in la_alignment_posteriors_windows (repeat_count and path_prob rows are zeroed too).  Argument errors (the
 * lattice entry's, a repeat_stride below max_labels with a repeat_from, a path_stride below max_frames with a path or path_prob,
 * path_prob without path, a negative or NaN repeat_penalty) are answered on the host under this entry's name before anything is
 * enqueued; never synchronises, allocates or frees.
 */
int la_alignment_posteriors_repeats_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_alignment_posteriors_repeats(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                    const int32_t *labels, int32_t labels_stride,
                                    const int32_t *n_labels, const int32_t *n_frames,
                                    int32_t batch, int32_t max_frames, int32_t max_labels,
                                    const int32_t *onset, const int32_t *offset, int32_t out_stride,
                                    int32_t boundary_window,
                                    const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                                    const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                    const int32_t *repeat_from, int32_t repeat_stride, double repeat_penalty,
                                    const int32_t *path, int32_t path_stride,
                                    float *occupancy, float *onset_prob, float *offset_prob, float *visits,
                                    float *span_skip_prob, float *repeat_count, float *path_prob,
                                    double *log_z, int32_t *status,
                                    float *gamma_out, int64_t gamma_batch_stride, int64_t gamma_row_stride,
                                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Whole-song confidence for repeated lyric lines: la_alignment_posteriors_repeats for up to 4095 labels.  The arguments are that
 * entry's, unchanged and in the same order, and so is the meaning of every output (expected counts included).
 * Up to 511 labels the call IS la_alignment_posteriors_repeats' sweep: the same kernel, the same workspace size, the same bits.
 * 512 .. 4095 labels: R = 2 / 4 / 8 lattice states per thread (up to 1023 / 2047 / 4095 labels), the same cell, so a clip gives the
 * same bits as in the lane-per-state form.  The workspace then holds, with NS = 1024 R,
 *     batch * max_frames * NS * 8   bytes of alpha rows,
 *   + batch * (NS / 2) * 6 * 8      bytes of sums (6 slots per label: occupancy, onset, offset, two span-skip halves, repeat_count),
 *   + batch * 3 NS * 4              bytes of arc lists (at most 4 arcs per optional span, at most 2 per repeat span)
 * -- la_alignment_posteriors_song_workspace_bytes -- and must be 16-byte aligned (at every label count).
 * More than 4095 labels: LA_EUNSUPPORTED, reported before the stride checks.  The other argument errors are
 * la_alignment_posteriors_repeats', answered on the host under this entry's name before anything is enqueued; never synchronises,
 * allocates or frees.  With repeat_from NULL or all -1 the outputs shared with la_alignment_posteriors_lattice are that entry's bit
 * for bit at every label count, visits equals its present_prob and repeat_count is 0.
 */
int la_alignment_posteriors_song_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_alignment_posteriors_song(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                 const int32_t *labels, int32_t labels_stride,
                                 const int32_t *n_labels, const int32_t *n_frames,
                                 int32_t batch, int32_t max_frames, int32_t max_labels,
                                 const int32_t *onset, const int32_t *offset, int32_t out_stride,
                                 int32_t boundary_window,
                                 const int32_t *skip_from, int32_t skip_stride, double skip_penalty,
                                 const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride,
                                 const int32_t *repeat_from, int32_t repeat_stride, double repeat_penalty,
                                 const int32_t *path, int32_t path_stride,
                                 float *occupancy, float *onset_prob, float *offset_prob, float *visits,
                                 float *span_skip_prob, float *repeat_count, float *path_prob,
                                 double *log_z, int32_t *status,
                                 float *gamma_out, int64_t gamma_batch_stride, int64_t gamma_row_stride,
                                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * Confidence for FREE LINE ORDER: the sum-product sweep of la_viterbi_lines_batch's lattice (same line_start / line_jump_penalty; no
 * counterpart in the reference).  States, jump sources, jump targets and the class rule are that entry's.  A path is one state per
 * frame; it weighs exp(sum_t e_t(path_t)) times one factor per transition, with q = exp(-line_jump_penalty):
 *   plain transitions weigh 1: k -> k, k -> k+1, and k -> k+2 into an odd state whose neighbour label differs;
 *   a jump weighs q: a transition source -> target that the class rule allows and that is not a plain transition already (the DP takes
 *       the free arc where both exist; no pair of states counts twice);
 *   start: states 0 and 1 weigh 1, every other target 2a+1 weighs q;  end: states S-1 and S-2 weigh 1, every other source but state 0 q.
 * la_alignment_posteriors' arguments through boundary_window, then line_start, line_stride, line_jump_penalty as la_viterbi_lines_batch,
 * then path [batch][path_stride] (that entry's output for the same lattice, with onset / offset its first visits; NULL = not given).
 * A path may visit a label any number of times: a VISIT is a maximal run of frames in one odd state, entry_t(n) / exit_t(n) are the
 * expected numbers of visits of label n that begin / end at frame t (a jump into 2a+1 is an entry of a and an exit of its source; a
 * start in an odd state is an entry at frame 0, an end in one an exit at the last frame), and what is summed from them are EXPECTED
 * COUNTS that can exceed 1; nothing is clamped.  Outputs:
 *   log_z, gamma_t(k), occupancy, onset_prob, offset_prob, gamma_out, path_prob[b][t] = gamma_t(path[b][t]) ([batch][path_stride], NULL =
 *       not wanted; LA_EINVAL without a path): as la_alignment_posteriors_repeats, about the reported (first) visit; 0 for a label never
 *       visited (onset -1);
 *   visits[b][n] = sum_t entry_t(n): the expected number of times label n is sung.  It is constant along a line: a path enters a line
 *       only at its start and leaves it only at its end;
 *   in_order[b][a], for a line start a: the expected number of visits of label a that begin in print order -- by the plain transition
 *       from 2a or, where the labels differ, from 2a-1, and for a = 0 also a start in state 1.  0 for every other label.
 *       visits - in_order at a line start is the expected number of arrivals out of print order: jumps plus free starts.
 *   status[b]: as la_alignment_posteriors; LA_EINVAL also for a clip whose line_start[0] is 0, LA_EINFEASIBLE where no path exists
 *       (+inf penalty and too few frames).  Rows of failed clips are zero, log_z 0 (-inf when infeasible); batch mates are unaffected.
 * Identities (tested): the rows of gamma sum to 1; with line_jump_penalty = +inf every shared output is la_alignment_posteriors', visits
 * 1 and in_order the line starts; with a single line they are la_alignment_posteriors_repeats' with repeat_from[0] = L_b and
 * repeat_penalty = line_jump_penalty, and visits[0] - in_order[0] its repeat_count[0] -- each within the bound below.
 * The M^2 jump arcs of M lines cost O(S + M) additions per frame and no subtraction (csrc/la_line_posterior.hip, DESIGN.md "Posteriors
 * on the line-order lattice"): path scores and the sums over sources are float64, a step's neighbour terms take their correction in
 * float32 as in la_alignment_posteriors; every probability, count and log_z within 8 T 2^-23 max(1, |value|) of a float64 evaluation.
 * The sums run in an order fixed by the kernel form: two calls, and a clip alone in the same form, agree bit for bit.
 * Up to 4095 labels (LA_EUNSUPPORTED above).  `workspace` (8-byte aligned, always needed) holds every alpha row, the jump term of every
 * label position and three sums per label position: batch * (max_frames * 1.5 S_pad + 1.5 S_pad) * 8 bytes, S_pad = 64 * the
 * smallest power of two of waves that holds 2 max_labels + 1 states up to 511 labels, 2048 / 4096 / 8192 up to 1023 / 2047 / 4095.
 * Argument errors (null pointers, strides, a negative or NaN penalty, path_prob without path) are answered on the host under this
 * entry's name before anything is enqueued; never synchronises, allocates or frees.
 */
int la_alignment_posteriors_lines_workspace_bytes(int32_t batch, int32_t max_frames, int32_t max_labels, size_t *bytes);

int la_alignment_posteriors_lines(const float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                  const int32_t *labels, int32_t labels_stride,
                                  const int32_t *n_labels, const int32_t *n_frames,
                                  int32_t batch, int32_t max_frames, int32_t max_labels,
                                  const int32_t *onset, const int32_t *offset, int32_t out_stride,
                                  int32_t boundary_window,
                                  const int32_t *line_start, int32_t line_stride, double line_jump_penalty,
                                  const int32_t *path, int32_t path_stride,
                                  float *occupancy, float *onset_prob, float *offset_prob,
                                  float *visits, float *in_order, float *path_prob,
                                  double *log_z, int32_t *status,
                                  float *gamma_out, int64_t gamma_batch_stride, int64_t gamma_row_stride,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- */
/* emission prep from materialised logits                                     */
/*   (replaces utils/alignment.py:123-134 [CTC] and :14-20 [plain])           */
/* ------------------------------------------------------------------------- */
/*
 * logits [batch][frames][vocab] float32 (device).  Computes the row normaliser
 * over the variant's column range and writes only the columns the DP reads:
 * em[b][t][0] and em[b][t][1+n] for n < n_labels[b] (compact layout above).
 */
int la_emissions_from_logits(const float *logits, int64_t batch_stride, int64_t row_stride,
                             int32_t batch, int32_t frames, int32_t vocab, int32_t variant,
                             const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                             int32_t max_labels,
                             float *em, int64_t em_batch_stride, int64_t em_row_stride, void *stream);

/* ------------------------------------------------------------------------- */
/* pronunciation alternatives: characters with several readings               */
/*   (addition; the reference maps every character to one class)              */
/* ------------------------------------------------------------------------- */
/*
 * A label position n of clip b may have a set of readings R_n = [labels[b][n], extra_1, ...] (class ids, the sheet's own class
 * first).  Its lattice state is scored on the MERGED class: em[t][1+n] = log sum_a exp(em_a[t]) over its readings, a per-frame
 * merge.  The emissions of every reading come from la_fc_emissions / la_emissions_from_logits run on the EXPANDED label list (all
 * readings of position 0, then of position 1, ...); the two entries below sit in front of and behind the lattice entries, which run
 * on the folded matrix unchanged.
 *
 * Expanded layout: em_x[b][t][0] is silence; columns 1 + alt_start[b][n] .. alt_start[b][n+1] are position n's readings in order.
 * alt_start (device) is a CSR row of n_labels[b] + 1 int32 per clip, alt_start[b][0] = 0, non-decreasing, alt_start[b][n_labels[b]]
 * <= max_columns; alt_stride is its row pitch in elements.  (Entries outside 0 .. max_columns are clamped into it, so a malformed
 * row reads no memory outside the expanded row; an empty group folds to -inf.)
 *
 * la_emissions_merge_readings: em[b][t][0] = em_x[b][t][0] bit for bit; a position with one reading is copied bit for bit; with
 * A >= 2 readings x_0 .. x_{A-1}: m = their float maximum, the result is -inf if m is -inf, otherwise
 *     (float)((double)m + log(sum_a exp((double)x_a - (double)m)))
 * summed in float64 in ascending a and rounded once.  Written: rows t < n_frames[b], columns 0 .. n_labels[b]; rows beyond, columns
 * beyond and the stride padding are left untouched.  Strides are in elements and arbitrary (rows need no alignment; em_x rows hold
 * max_columns + 1, em rows max_labels + 1 entries); em must not overlap em_x.  One read of the expanded rows, one write of the folded
 * rows; no atomics and nothing shared between clips, so a clip's bits are the same alone and in a batch.
 *
 * la_reading_scores: which reading was sung, decided on the boundaries the DP chose (onset / offset [batch][out_stride], the lattice
 * entries' outputs; with repeat spans the reported, first visit).  col_score[b][j] for every expanded column j <
 * alt_start[b][n_labels[b]] = the float64 sum of em_x[b][t][1+j] over t ascending in [onset, offset) of the column's position: the
 * segment's log-likelihood had the character been that reading throughout (sequential, so two calls agree bit for bit).
 * reading[b][n] = the smallest a (0 = the sheet's own class) with the largest col_score[b][alt_start[b][n] + a].  A skipped position
 * (onset -1) gets reading -1 and scores 0.  col_score rows hold max_columns doubles (col_stride), reading rows max_labels int32.
 *
 * Both: batch, max_frames, max_labels <= 0, a null pointer, max_columns < max_labels or a stride smaller than its width ->
 * LA_EINVAL; more than 4095 labels or columns -> LA_EUNSUPPORTED (reported before the stride checks); answered on the host under the
 * entry's name before anything is enqueued.  Neither entry synchronises, allocates or frees.
 */
int la_emissions_merge_readings(const float *em_x, int64_t emx_batch_stride, int64_t emx_row_stride,
                                const int32_t *alt_start, int32_t alt_stride,
                                const int32_t *n_labels, const int32_t *n_frames,
                                int32_t batch, int32_t max_frames, int32_t max_labels, int32_t max_columns,
                                float *em, int64_t em_batch_stride, int64_t em_row_stride, void *stream);

int la_reading_scores(const float *em_x, int64_t emx_batch_stride, int64_t emx_row_stride,
                      const int32_t *alt_start, int32_t alt_stride, const int32_t *n_labels,
                      const int32_t *onset, const int32_t *offset, int32_t out_stride,
                      int32_t batch, int32_t max_frames, int32_t max_labels, int32_t max_columns,
                      double *col_score, int32_t col_stride, int32_t *reading, int32_t reading_stride, void *stream);

/* ------------------------------------------------------------------------- */
/* pronunciation scores: was the sheet's character the one that was sung?     */
/*   (addition; "goodness of pronunciation" of forced aligners)               */
/* ------------------------------------------------------------------------- */
/*
 * The lattice forces every state onto its sheet class; the confidences above are posteriors GIVEN the sheet.  la_segment_class_scores
 * looks at the segment the DP gave a position and asks which class was heard there: it sums the emissions of n_cand candidate classes
 * over the segment, ranks the position's own class among them and names the top_k best.
 *
 * em_c[b][t][j] (device, float32) is the emission of candidate class j at frame t; strides in elements and arbitrary -- in practice a
 * column window of a wider compact emission matrix, so rows need no alignment (rows hold n_cand entries).  onset / offset
 * [batch][out_stride] are a lattice entry's outputs (frames; -1 = skipped; with repeat spans the reported, first visit); own_col
 * [batch][own_stride] names the candidate column that holds position n's own class (-1 or outside 0 .. n_cand-1: none).
 *
 * Per position n < n_labels[b] with onset >= 0 (all candidates share the segment [t0, t1) = [min(onset, max_frames),
 * max(t0, min(offset, max_frames)))):
 *   seg_score[b][n][j]  (optional, null = not wanted) = the float64 sum of em_c[b][t][j] over t ascending in [t0, t1): sequential, so
 *                       two calls agree bit for bit and a clip's bits are the same alone and in a batch;
 *   top_col / top_score [b][n][k], k < top_k: the candidates with the largest sums, the largest first, ties to the smaller column;
 *                       where top_k > n_cand the trailing entries are -1 / -inf;
 *   own_score[b][n]     = the sum of column own_col (0 without one);
 *   own_rank[b][n]      = the number of candidates with a larger sum, or an equal sum and a smaller column (0 = the own class is the
 *                       best; -1 without an own column);
 *   n_seg_frames[b][n]  = t1 - t0.
 * A skipped position (onset < 0) gets top_col -1, top_score 0, own_score 0, own_rank -1, n_seg_frames 0 and, where seg_score is given,
 * a row of zeros.  -inf and clipped (-1000) emissions are ordinary values.  Positions n >= n_labels[b], and every stride's padding,
 * are left untouched.  n_labels, onset, offset and own_col are device data and are clamped in the kernel (n_labels into 0 ..
 * max_labels, frames into 0 .. max_frames), so a malformed row reads nothing outside its clip.
 *
 * Layout of the outputs: seg_score rows at b * seg_batch_stride + n * seg_row_stride (n_cand doubles each); top_col / top_score rows
 * at (b * max_labels + n) * top_stride (top_k entries each); own_score / own_rank / n_seg_frames share out_stride with onset / offset.
 *
 * batch, max_frames, max_labels, n_cand or top_k <= 0, a null pointer (seg_score excepted) or a stride smaller than its width ->
 * LA_EINVAL; max_labels or n_cand above 4095, top_k above 16 (or more than 65535 clips) -> LA_EUNSUPPORTED, reported before the
 * stride checks; answered on the host under the entry's name before anything is enqueued.  The segments of a clip are disjoint, so a
 * call reads every emission at most once.  The entry does not synchronise, allocate, free or use atomics.
 */
int la_segment_class_scores(const float *em_c, int64_t emc_batch_stride, int64_t emc_row_stride,
                            const int32_t *n_labels, const int32_t *onset, const int32_t *offset, int32_t out_stride,
                            const int32_t *own_col, int32_t own_stride,
                            int32_t batch, int32_t max_frames, int32_t max_labels, int32_t n_cand, int32_t top_k,
                            double *seg_score, int64_t seg_batch_stride, int64_t seg_row_stride,
                            int32_t *top_col, double *top_score, int32_t top_stride,
                            double *own_score, int32_t *own_rank, int32_t *n_seg_frames,
                            void *stream);

/* ------------------------------------------------------------------------- */
/* off-sheet slots: singing that is in the audio but not on the sheet         */
/*   (addition; the wildcard / "star" label of other forced aligners)         */
/* ------------------------------------------------------------------------- */
/*
 * A slot is an ordinary label position of the lattice whose emission column holds "this frame is voiced, whatever the class", made
 * skippable by a one-label optional span; the lattice entries run unchanged.  Both emission providers (la_fc_emissions /
 * la_align_head_forward and la_emissions_from_logits) leave log P(silence), clamped at -1000, in column 0 of the compact matrix in
 * both variants, and the slot's emission is a function of that column alone:
 *     v   = log(-expm1((double)em[b][t][0])) - penalty        log P(frame is not silence) - penalty, float64
 *     out = v > -1000.0 ? (float)v : -1000.0f                 rounded once; v NaN or -inf (em NaN or >= 0): the floor
 *     em[b][t][1 + x] = out     for every x = slot_cols[b][i], i < n_slots[b], and every t < n_frames[b]
 * A sheet character's emission is log p_c + log P(voiced) (CTC variant; plain: log p_c), so the slot beats the sheet's character on a
 * frame exactly when that character holds less than exp(-penalty) of the voiced probability.
 *
 * la_emissions_offsheet_columns writes in place.  em may be a column window of a wider matrix: strides are in elements and taken as
 * given (rows hold max_labels + 1 entries and need no alignment).  slot_cols [batch][slot_stride] (device) holds label positions,
 * 0-based and ascending; an entry outside 0 .. max_labels-1 is skipped and never used as an index; n_slots / n_frames (device) are
 * clamped into 0 .. max_slots / 0 .. max_frames.  Rows t >= n_frames[b], every other column and clips with n_slots[b] = 0 are not
 * touched.  The float64 transcendentals are evaluated once per row; no atomics and nothing shared between clips, so a clip's bits are
 * the same alone and in a batch and two calls agree bit for bit.  (Subnormal float32 inputs convert by the flush mode: unspecified.)
 *
 * A null pointer, batch / max_frames / max_labels / max_slots <= 0, a negative or NaN penalty, em_row_stride < max_labels + 1 or
 * slot_stride < max_slots -> LA_EINVAL; more than 4095 labels (or more than 65535 clips) -> LA_EUNSUPPORTED, reported before the
 * stride checks; answered on the host under the entry's name before anything is enqueued.  The entry does not synchronise, allocate
 * or free.
 */
int la_emissions_offsheet_columns(float *em, int64_t em_batch_stride, int64_t em_row_stride,
                                  const int32_t *slot_cols, int32_t slot_stride, const int32_t *n_slots, const int32_t *n_frames,
                                  int32_t batch, int32_t max_frames, int32_t max_labels, int32_t max_slots, double penalty,
                                  void *stream);

/* ------------------------------------------------------------------------- */
/* log-mel front end  (replaces whisper.audio.log_mel_spectrogram + pad_or_trim, */
/*                      call sites module/align_model.py:84,89,100,109)           */
/* ------------------------------------------------------------------------- */
/*
 * audio [batch][n_samples] float32 -> mel [batch][80][n_frames], n_frames =
 * n_samples / 160, float32.  The "-8" floor uses the max over the WHOLE batch
 * tensor, as upstream whisper does.  mel_filters is the [80][201] Slaney table
 * (device), window the 400-tap periodic Hann (device).  These names are the 80-bin
 * forms (whisper tiny .. large-v2); the *_n entries below take the bin count (80 or
 * 128, the large-v3 generation).
 */
int la_logmel_workspace_bytes(int32_t batch, int32_t n_samples, size_t *bytes);
int la_logmel_f32(const float *audio, int32_t batch, int32_t n_samples,
                  const float *mel_filters, const float *window,
                  float *mel, int64_t mel_batch_stride, int64_t mel_row_stride,
                  void *workspace, size_t workspace_bytes, void *stream);
/*
 * The same with the constants (windowed DFT matrix in MFMA fragment order, padded
 * filter bank) built once per (mel_filters, window) pair into a caller-owned
 * device buffer of la_logmel_constants_bytes(): 2 launches per call instead of 3.
 * whisper builds its window and loads its filter asset once per process the same
 * way (whisper.audio.mel_filters is lru-cached).
 */
int la_logmel_constants_bytes(size_t *bytes);
int la_logmel_constants(const float *mel_filters, const float *window,
                        void *consts, size_t consts_bytes, void *stream);
int la_logmel_f32_prepared(const float *audio, int32_t batch, int32_t n_samples,
                           const void *consts,
                           float *mel, int64_t mel_batch_stride, int64_t mel_row_stride,
                           void *workspace, size_t workspace_bytes, void *stream);
/*
 * Ragged form (an addition: upstream pads a batch to its longest clip BEFORE the log-mel and floors at the batch maximum, which
 * la_logmel_* reproduce).  Clip b = the first n_samples[b] (device int32 [batch]) samples of row b of audio [batch][max_samples].
 * mel [batch][80][out_frames] receives, per clip, what la_logmel_f32_prepared gives for that clip ALONE -- reflect padding at the
 * clip's own end, n_samples[b] / 160 frames, floor at the clip's own maximum - 8 -- followed by literal zeros up to out_frames
 * (= pad_or_trim; out_frames >= max_samples / 160, 3000 for the encoder).  Tiles wholly past a clip's end do no DFT.  2 launches.
 * Every n_samples[b] must be > 200 (reflect padding; the caller checks it: the array lives on the device) and <= max_samples
 * (larger values are clamped).  max_samples <= 200 is refused.  Workspace: la_logmel_ragged_workspace_bytes(batch, max_samples),
 * 256-byte aligned.
 */
int la_logmel_ragged_workspace_bytes(int32_t batch, int32_t max_samples, size_t *bytes);
int la_logmel_ragged_f32_prepared(const float *audio, const int32_t *n_samples, int32_t batch, int32_t max_samples,
                                  const void *consts,
                                  float *mel, int64_t mel_batch_stride, int64_t mel_row_stride, int32_t out_frames,
                                  void *workspace, size_t workspace_bytes, void *stream);
/*
 * The same six with the mel bin count as their first argument (an addition: the reference calls whisper's log-mel with its default of
 * 80 bins).  n_mels = 80 (whisper tiny .. large-v2) or 128 (large-v3, large-v3-turbo); anything else is LA_EINVAL before any launch.
 * mel_filters is [n_mels][201], mel [batch][n_mels][frames].  With n_mels = 80 each entry IS the entry above it is named after (those
 * are its n_mels = 80 call): the same launches, the same bits.  la_logmel_workspace_bytes_n serves the dense and the ragged form (the
 * one-call form keeps its constants in the workspace, so the size grows with n_mels).
 * Constants belong to ONE bin count, and the prepared entries check it on the host, by the buffer's address: la_logmel_constants_n
 * (and la_logmel_constants) record (consts, n_mels) once their launch is accepted; a later call on the same address replaces the
 * record.  A prepared entry with n_mels = 128 takes only an address recorded for 128.  One with n_mels = 80 refuses an address
 * recorded for 128 and takes every other (a copy of an 80-bin buffer has no record, and la_logmel_f32_prepared has always taken it).
 * So: build 128-bin constants in the buffer they are used from, and do not reuse that address for a copy of 80-bin constants without
 * building them there.  The refusal is LA_EINVAL before any launch; nothing on the device is read for it.
 */
int la_logmel_constants_bytes_n(int32_t n_mels, size_t *bytes);
int la_logmel_constants_n(int32_t n_mels, const float *mel_filters, const float *window,
                          void *consts, size_t consts_bytes, void *stream);
int la_logmel_workspace_bytes_n(int32_t n_mels, int32_t batch, int32_t n_samples, size_t *bytes);
int la_logmel_f32_n(int32_t n_mels, const float *audio, int32_t batch, int32_t n_samples,
                    const float *mel_filters, const float *window,
                    float *mel, int64_t mel_batch_stride, int64_t mel_row_stride,
                    void *workspace, size_t workspace_bytes, void *stream);
int la_logmel_f32_prepared_n(int32_t n_mels, const float *audio, int32_t batch, int32_t n_samples,
                             const void *consts,
                             float *mel, int64_t mel_batch_stride, int64_t mel_row_stride,
                             void *workspace, size_t workspace_bytes, void *stream);
int la_logmel_ragged_f32_prepared_n(int32_t n_mels, const float *audio, const int32_t *n_samples, int32_t batch,
                                    int32_t max_samples, const void *consts,
                                    float *mel, int64_t mel_batch_stride, int64_t mel_row_stride, int32_t out_frames,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- */
/* building blocks of embed_audio / align_rnn                                */
/* ------------------------------------------------------------------------- */
/* epilogue flags for la_gemm */
enum {
    LA_EPI_BIAS = 1,      /* + bias[n] (f32)                                          */
    LA_EPI_GELU = 2,      /* GELU after the bias.  f32 results (float32 mode, LA_EPI_OUT_F32): the erf form, |error| <= 1.2e-7.
                           * 16-bit results: x * sigmoid(x (a + b x^2 + c x^4)), a minimax fit to x Phi(x): max ABSOLUTE error 2.5e-5
                           * (below half a bf16 ulp for |gelu| >= 1e-2; the relative error is unbounded in the negative tail, where
                           * |gelu| < 1e-2 -- whisper's F.gelu is the erf form).  LA_EPI_GELU_ERF selects the erf form there too. */
    LA_EPI_RESIDUAL = 4,  /* + residual[m][n] (f32, own strides; batch stride may be 0) */
    LA_EPI_OUT_F32 = 8,   /* C is f32 regardless of the operand dtype                 */
    LA_EPI_MISH = 16,     /* x * tanh(softplus(x)) after the bias                     */
    LA_EPI_RES_GELU_GRAD = 32, /* la_gemm_f16x2 only, with LA_EPI_RESIDUAL: the result is MULTIPLIED by gelu'(residual[m][n]) instead of having
                           * it added -- the input gradient of the MLP's second Linear times the GELU derivative at the saved
                           * pre-activation (la_gelu_bwd_f32 without its pass over the [rows][4 d] buffer) */
    LA_EPI_GELU_ERF = 4096, /* with LA_EPI_GELU and a 16-bit result: the erfc-based form (max absolute error 1.3e-6, 20 x closer to
                           * F.gelu than the sigmoid fit) at ~40 % more epilogue issue slots.  (LA_GELU_PK=1 in the environment sets
                           * it on every launch: the developer A/B switch.) */
    /* operand layout flags of la_gemm_ex (float32 only), OR-ed into the same word: the operand is stored TRANSPOSED,
     * [K][rows] with pitch lda / ldw >= rows (rows % 4 == 0).  With a flag set K may be any length (a K-contiguous operand
     * must then have a pitch >= K rounded up to 32; what lies behind column K is read and ignored, NaN and Inf included);
     * both set = the weight-gradient shape
     * dW[n][k] = sum_m dY[m][n] X[m][k], which reads dY and X as they are.  Replaces a transpose pass per operand. */
    LA_GEMM_TRANS_A = 512,
    LA_GEMM_TRANS_W = 1024
};

/*
 * C[z][m][n] = epi( sum_k A[z][m][k] * W[n][k] ),  z < batch.
 * A: `dtype`, row stride lda (elements; may be < K: the conv-as-GEMM views
 * overlap rows), batch stride strideA.  W: `dtype`, [N][K] row-major (nn.Linear
 * layout).  C: `dtype` (or f32 with LA_EPI_OUT_F32), row stride ldc, batch
 * stride strideC.  K % 64 == 0 (bf16) / K % 32 == 0 (f32); A, W, C 16-byte aligned;
 * M, N arbitrary (edge tiles are predicated).
 * Replaces every nn.Linear / nn.Conv1d of whisper.model.AudioEncoder and the
 * GRU input projections of module/align_model.py:23-28.
 */
int la_gemm(int32_t dtype, int32_t M, int32_t N, int32_t K, int32_t batch,
            const void *A, int64_t lda, int64_t strideA,
            const void *W,
            void *C, int64_t ldc, int64_t strideC,
            const float *bias,
            const float *residual, int64_t ldr, int64_t strideR,
            int32_t epilogue, void *stream);

/* y[m][:] = LayerNorm(x[m][:]) * gamma + beta, eps 1e-5; x f32 [M][d], y `out_dtype`. */
int la_layernorm(const float *x, int64_t ldx, int32_t M, int32_t d,
                 const float *gamma, const float *beta,
                 void *y, int64_t ldy, int32_t out_dtype, void *stream);

/*
 * Non-causal multi-head self-attention over packed QKV rows.
 * qkv [batch*frames][3*n_head*64] (`dtype`): columns [q | k | v], head h at
 * h*64; q is expected PRE-SCALED by head_dim^-0.5 (folded into the projection
 * weights at pack time; the reference scales q and k by head_dim^-0.25 each,
 * whisper MultiHeadAttention.qkv_attention).  softmax in f32.
 * out [batch*frames][n_head*64] (`dtype`).  head_dim is 64 for every Whisper size.
 */
int la_attention(int32_t dtype, const void *qkv, int64_t ld_qkv, void *out, int64_t ld_out,
                 int32_t batch, int32_t frames, int32_t n_head, void *stream);

/* General form for the Whisper text decoder (whisper.model.TextDecoder; module/align_model.py:118-121): separate
 * q [batch*q_len][>= n_head*64] and k / v [batch*kv_len][>= n_head*64] row sets (k and v share ld_kv), q pre-scaled.
 * causal != 0: key j is visible to query i iff j <= i (decoder self-attention; requires q_len == kv_len). */
int la_attention_ex(int32_t dtype, const void *q, int64_t ld_q, const void *k, const void *v, int64_t ld_kv,
                    void *out, int64_t ld_out, int32_t batch, int32_t q_len, int32_t kv_len, int32_t n_head,
                    int32_t causal, void *stream);

/* Attention against a key / value cache (autoregressive decoding: the next row of SURVEY 8f, inference_transcript.py): clip
 * b's keys / values are rows [b*kv_batch_rows, b*kv_batch_rows + kv_len) of k / v (the cache holds kv_batch_rows >= kv_len
 * rows per clip), its queries rows [b*q_batch_rows, +q_len) of q, out rows are packed [b*q_len + i].  causal with q_len == 1
 * (one new token) needs no mask; causal with q_len == kv_len is la_attention_ex's mask. */
int la_attention_cached(int32_t dtype, const void *q, int64_t ld_q, int64_t q_batch_rows, const void *k, const void *v,
                        int64_t ld_kv, int64_t kv_batch_rows, void *out, int64_t ld_out, int32_t batch, int32_t q_len,
                        int32_t kv_len, int32_t n_head, int32_t causal, void *stream);

/* out[r] = argmax_c x[r][c] (first maximum), int64: the greedy token choice over the decoder logits. */
int la_argmax_rows_f32(const float *x, int64_t ld, int32_t rows, int32_t cols, int64_t *out, void *stream);

/* The k (<= 8) largest values of each row, their indices (first maximum on ties) and the row's log-sum-exp:
 * log-probability of candidate j = vals[r][j] - lse[r] (beam search over the decoder logits). */
int la_topk_rows_f32(const float *x, int64_t ld, int32_t rows, int32_t cols, int32_t k, float *vals, int64_t *idx, float *lse,
                     void *stream);

/* x[b*n_tok + i][:] = token_embedding[tokens[b][i]][:] + positional_embedding[i][:]   (f32 tables, f32 out);
 * TextDecoder.forward's first line.  tokens int64 [batch][n_tok]. */
int la_embed_tokens(const int64_t *tokens, int32_t batch, int32_t n_tok, const float *token_embedding, int32_t n_vocab,
                    const float *positional_embedding, int32_t d, float *x, void *stream);

/* mel [batch][n_mels][frames] f32 -> channels-last zero-padded rows for the conv-as-GEMM view:
 * out[b][1 + t][c] (`dtype`), row pitch `c_pad`, (frames + 2) rows per clip, rows 0 and frames+1
 * and channels >= n_mels zeroed. */
int la_mel_to_rows(const float *mel, int64_t mel_batch_stride, int64_t mel_row_stride,
                   int32_t batch, int32_t n_mels, int32_t frames,
                   void *out, int32_t c_pad, int32_t dtype, void *stream);

/*
 * One bidirectional GRU layer recurrence (nn.GRU gate order r,z,n;
 * module/align_model.py:23-28).  gi [batch][frames][2][3H] f32 holds the input
 * projections W_ih x + b_ih of both directions; w_hh [2][3H][H] (`dtype`),
 * b_hh [2][3H] f32.  out [batch][frames][2H] (`dtype`) receives h_t (forward in
 * columns 0..H-1, reverse in H..2H-1); out_mish (optional, same shape) receives
 * Mish(h_t) (module/align_model.py:37).  Persistent kernel: 2 * H/128 (16-bit modes, H % 128 == 0, H <= 384; else 2 * H/64) workgroups
 * per 16 clips exchange h in `workspace` (zeroed on the stream by this call): by default as data-tagged 8-byte granules
 * {h, h | step} polled by the consumers (16-bit modes; option gru_handoff = 1: through `out` with write-through (sc1)
 * stores and per-step arrival counters).  H % 64 == 0;
 * at most 224 workgroups may be co-resident (16-bit modes, H=384: 8-wave workgroups, 2 * 3 per 16 clips).
 * dtype LA_F32, more than 4 clips, option x2_inference = 1 (round 6): the recurrent product h W_hh^T runs as three f16 MFMA products
 * over split operands at float32 accuracy (W_hh rows scaled and split into two half fragment sets resident in registers, h exchanged as
 * {hi | lo, step} granules): 4.4 instead of 11.4 us per step at 16 clips; fewer clips keep the float32 kernel's v_fma path.
 * `timeout_flag` (device int32, optional) is set non-zero if a bounded wait (option gru_timeout_us, default 3 s) gave up: the launch set was
 * not co-resident and `out` is garbage.  Recover by calling again after hipDeviceSynchronize (alone on the device the set is co-resident);
 * INTEGRATION.md "GRU time-out and recovery".
 * Statuses, answered on the host before anything is enqueued (the same in la_gru_layer, la_gru_layer_ragged, la_gru_layer_train_fwd and
 * la_gru_layer_bwd): batch == 0 or frames == 0 -> LA_OK, nothing is looked at.  LA_EINVAL: a null pointer (timeout_flag and out_mish
 * excepted), a bad dtype, a negative batch / frames or hidden <= 0, w_hh / out / workspace (backward: dgh / workspace) not 16-byte aligned,
 * a workspace below la_gru_workspace_bytes.  LA_EUNSUPPORTED: a well-formed shape the kernels are not built for -- hidden not a multiple
 * of 64 or beyond the type's limit (float32 384, 16-bit 512, backward 384), or more than 224 co-resident workgroups (split the batch).
 * la_gru_workspace_bytes: [16-byte header][arrival counters [ceil(batch / 16)][2][frames] u32] padded to 256 bytes, then the granule ring,
 * the larger of ceil(batch / 16) * 64 * hidden * 8 bytes (forward) and, for hidden % 64 == 0, ceil(batch / 16) * 64 * (hidden / 64)^2 * 512
 * bytes (backward); LA_EINVAL for a null result or a non-positive size.
 */
int la_gru_workspace_bytes(int32_t batch, int32_t frames, int32_t hidden, size_t *bytes);
int la_gru_layer(int32_t dtype, const float *gi, const void *w_hh, const float *b_hh,
                 void *out, void *out_mish, int32_t batch, int32_t frames, int32_t hidden,
                 void *workspace, size_t workspace_bytes, int32_t *timeout_flag, void *stream);
/*
 * The same recurrence over clips of different lengths: n_frames [batch] (device int32), 0 <= n_frames[b] <= frames = the launch's
 * maximum.  Rows t < n_frames[b] of out / out_mish are what la_gru_layer gives for clip b alone over n_frames[b] frames (the reverse
 * direction enters frame n_frames[b] - 1 with h = 0); rows t >= n_frames[b] are unspecified.  Every inference form takes it (float32
 * v_fma / MFMA and f16x2 forms, 16-bit counter and granule forms) as a compile-time variant of its kernel: after the gate arithmetic
 * a lane SELECTS h = 0 at steps past its clip's end (gi there may hold anything, NaN included); the hand-off protocol, the time-out
 * flag and the workspace are la_gru_layer's, and every clip of the launch still takes `frames` steps.  la_gru_layer itself launches
 * the kernels it launched before.
 */
int la_gru_layer_ragged(int32_t dtype, const float *gi, const void *w_hh, const float *b_hh,
                        void *out, void *out_mish, int32_t batch, int32_t frames, const int32_t *n_frames, int32_t hidden,
                        void *workspace, size_t workspace_bytes, int32_t *timeout_flag, void *stream);

/*
 * Fused head tail: Linear(2H -> V) + emission prep, WITHOUT materialising the
 * [batch][frames][V] logits (replaces module/align_model.py:38 followed by
 * utils/alignment.py:123-134 / :14-20 and the device->host copy at
 * inference_alignment.py:161).  act [batch*frames][2H] (`dtype`) = Mish(GRU out);
 * w_fc [V][2H] (`dtype`), b_fc [V] f32.  Writes compact emissions (layout above).
 */
int la_fc_emissions_workspace_bytes(int32_t dtype, int32_t batch, int32_t frames, int32_t in_dim, int32_t vocab,
                                    int32_t max_labels, size_t *bytes);
int la_fc_emissions(int32_t dtype, const void *act, int64_t ld_act, const void *w_fc, const float *b_fc,
                    int32_t batch, int32_t frames, int32_t in_dim, int32_t vocab, int32_t variant,
                    const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                    int32_t max_labels,
                    float *em, int64_t em_batch_stride, int64_t em_row_stride,
                    void *workspace, size_t workspace_bytes, void *stream);
/* la_fc_emissions for FLOAT32 rows with the normaliser product (the full [batch*frames] x V Linear) on the f16 matrix pipe at float32
 * accuracy: w_fc_x2 / w_fc_x2s = W_fc as f16x2 planes [V][2][in_dim] (la_split_f16x2, kp = in_dim) and their per-row inverse scales; act is split
 * inside (workspace).  Same results to float32 accuracy; shapes outside the 256 x 256 kernel's domain (in_dim % 128, < 192 tiles) take
 * la_fc_emissions' float32 kernel. */
int la_fc_emissions_x2_workspace_bytes(int32_t batch, int32_t frames, int32_t in_dim, int32_t vocab, int32_t max_labels, size_t *bytes);
int la_fc_emissions_x2(const float *act, int64_t ld_act, const float *w_fc, const float *b_fc, const void *w_fc_x2, const float *w_fc_x2s,
                       int32_t batch, int32_t frames, int32_t in_dim, int32_t vocab, int32_t variant,
                       const int32_t *labels, int32_t labels_stride, const int32_t *n_labels, int32_t max_labels,
                       float *em, int64_t em_batch_stride, int64_t em_row_stride, void *workspace,
                       size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- */
/* fine-tune path: losses on the align logits and the optimizer step          */
/* ------------------------------------------------------------------------- */
/*
 * compute_ce_loss(compute_sil=True) + compute_ctc_loss (train_multitask.py:587-633), forward and gradient with
 * respect to the logits.  logits [batch][frames][row_stride >= vocab+1] f32: columns 0..vocab-1 are the word classes
 * (column 0 = CTC blank), column `vocab` the silence logit (vocab = 21128 in the reference).
 *   frame_labels [batch*frames] i32: class id (>= 1) of the frame or -100 (already trimmed / padded to `frames`,
 *                train_multitask.py:596-603); the reference's "-1" shift (:607) is folded into the column choice.
 *   ctc_labels [batch][labels_stride] i32 class ids, n_labels[b] of them valid (target_length, :629).
 * losses[0] = word CE (mean over frames with a label), losses[1] = silence BCE (mean over all frames),
 * losses[2] = CTC (mean over the batch of nll_b / n_labels[b]; +inf if an utterance is infeasible).
 * dlogits (optional, same layout) receives scale * d(losses[0]+losses[1]+losses[2]) / dlogits, restricted to the
 * requested terms (use_ce / use_ctc).  The alpha/beta lattice runs one workgroup per utterance, one lane per state.
 * The losses of a term that was not requested are not meaningful.
 *   - A clip with n_labels[b] = 0 contributes 0 to losses[2] and nothing to the gradient; the sum is still divided by `batch`.
 *   - A frame label outside 1..vocab-1 other than -100 is ignored by the word CE (not counted, no gradient); for the silence BCE it
 *     is a frame with a label (target 0).  With no frame label in 1..vocab-1 at all, losses[0] is NaN and the word-CE gradient zero.
 *   - A CTC label whose class lies outside 0..vocab-1 can be emitted by no frame: the clip is infeasible, like one with fewer frames
 *     than labels plus adjacent repeats (losses[2] = +inf; the clip's CTC gradient rows are exact zeros, its batch mates unaffected).
 *   - n_labels[b] <= max_labels is the caller's duty (it is not checked: the labels live on the device); max_labels <= 511.
 *   - The CTC gradient of a class that occurs at several label positions is summed with float atomics: where a class repeats,
 *     dlogits is not bit-reproducible from call to call.
 * Each row's normaliser is kept as its maximum and the log of the sum apart, (x - m) - log s, so a common offset on a row costs nothing.
 * workspace: la_multitask_loss_workspace_bytes, 256-byte aligned.  Argument errors are answered before anything is enqueued.
 */
int la_multitask_loss_workspace_bytes(int32_t batch, int32_t frames, int32_t max_labels, size_t *bytes);
int la_multitask_loss(const float *logits, int64_t batch_stride, int64_t row_stride, int32_t batch, int32_t frames,
                      int32_t vocab, const int32_t *frame_labels, const int32_t *ctc_labels, int32_t labels_stride,
                      const int32_t *n_labels, int32_t max_labels, int32_t use_ce, int32_t use_ctc, float scale,
                      float *losses, float *dlogits, int64_t d_batch_stride, int64_t d_row_stride,
                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * Training from line times (addition; the reference has none): the negative log-partition of the lattice with per-state frame
 * windows as a loss on the align logits, forward and gradient with respect to the logits.  logits as in la_multitask_loss
 * ([batch][frames][row_stride >= vocab+1] f32, column `vocab` the silence logit); labels, n_labels, n_frames (NULL: every clip
 * has `frames` rows), skip_from / skip_stride / skip_penalty (skip_from may be NULL: no span anywhere), win_lo / win_hi /
 * win_stride and the 511-label limit as in la_alignment_posteriors_windows.
 *   em      = the CTC-variant compact emissions of la_emissions_from_logits (bit for bit):
 *             em[t][0] = logsigmoid(x[t][V]), em[t][1+n] = x[t][c_n] - lse_{1..V-1}(x[t]) + logsigmoid(-x[t][V]),  V = vocab
 *   nll[b]  = -log_z[b], the windowed log-partition of la_alignment_posteriors_windows on em
 *   loss[0] = (1 / batch) * sum over feasible b of nll[b] / n_frames[b]
 *   dlogits (optional) = scale * d loss / d logits: with gamma_t(s) the windowed posterior, g_sil = sum over even s of gamma_t(s),
 *             g_n = gamma_t(2n+1), g_voiced = sum_n g_n, w = scale / (batch * n_frames[b]):
 *               d[t][0] = 0
 *               d[t][c] = w * (g_voiced * softmax_{1..V-1}(x[t])[c] - sum over n with c_n = c of g_n),   1 <= c < V
 *               d[t][V] = w * (sigmoid(x[t][V]) - g_sil)
 *             rows t >= n_frames[b] are exact zeros; columns past V are not written.  The -1000 clip of the emission prep is
 *             treated as inactive (an emission that reaches it takes the gradient of the unclipped expression); a label whose
 *             class lies outside 1..V-1 (constant emission -1000) takes no part in the gradient.  Jump arcs of optional spans
 *             weigh a constant: they change gamma, not the formula.
 * status[b]: LA_OK; LA_EINFEASIBLE (no path inside the windows, or too few frames for the labels) and LA_EEMPTY (no label):
 * nll[b] = +inf, zero gradient rows, and the clip is left out of the sum, which is still divided by `batch`.
 * Deterministic: no float atomics, classes that occur at several label positions are summed in ascending position; a clip's
 * rows do not depend on its batch mates.  Argument errors (null pointers, strides, vocab < 3, a negative or NaN penalty; more
 * than 511 labels: LA_EUNSUPPORTED) are answered before anything is enqueued.  Never synchronises, allocates or frees.
 * workspace: 256-byte aligned.
 */
int la_anchored_alignment_loss_workspace_bytes(int32_t batch, int32_t frames, int32_t max_labels, size_t *bytes);
int la_anchored_alignment_loss(const float *logits, int64_t batch_stride, int64_t row_stride, int32_t batch, int32_t frames,
                               int32_t vocab, const int32_t *labels, int32_t labels_stride, const int32_t *n_labels,
                               const int32_t *n_frames, int32_t max_labels, const int32_t *skip_from, int32_t skip_stride,
                               double skip_penalty, const int32_t *win_lo, const int32_t *win_hi, int32_t win_stride, float scale,
                               float *loss, double *nll, int32_t *status, float *dlogits, int64_t d_batch_stride,
                               int64_t d_row_stride, void *workspace, size_t workspace_bytes, void *stream);

/*
 * clip_grad_norm_(params, max_norm) + AdamW on flat f32 buffers (train_multitask.py:337-340,683-686).
 * la_grad_sqnorm_f32 ADDS sum(grad^2) into *sum_sq (device double; zero it once, call it per bucket, all-reduce is the
 * caller's: gradients are already averaged over ranks before this).  la_adamw_step_f32 applies
 *   g' = g * grad_prescale * min(1, max_norm / (sqrt(*clip_sum_sq) * grad_prescale + 1e-6))    (clip_sum_sq may be NULL)
 *   p *= 1 - lr*wd;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 */
int la_grad_sqnorm_f32(const float *grad, int64_t n, double *sum_sq, void *stream);
int la_adamw_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int32_t step,
                      const double *clip_sum_sq, float max_norm, float grad_prescale, void *stream);

/*
 * Backward pass of the head (GRU x2 bidirectional -> Mish -> Linear, module/align_model.py:11-40), float32.
 * la_gru_layer_train_fwd = la_gru_layer(LA_F32) that also stores, per step, r, z, n and (W_hn h + b_hn) into
 * gates [batch][frames][2][4H].  la_gru_layer_bwd sweeps the recurrence backwards: dout = gradient w.r.t. the layer
 * output [batch][frames][2H]; writes dgi / dgh [batch][frames][2][3H], the gradients w.r.t. the input / recurrent gate
 * pre-activations, from which the weight gradients are plain GEMMs (dW_ih = dgi^T x, dW_hh = dgh^T h_prev, dx = dgi W_ih).
 * The helpers below express those GEMMs for la_gemm (both operands K-contiguous): zero-padded transposes, column sums
 * (bias gradients), Mish forward / backward, masked scaling (the inter-layer dropout of nn.GRU in train mode).
 */
int la_gru_layer_train_fwd(const float *gi, const float *w_hh, const float *b_hh, float *out, float *gates,
                           int32_t batch, int32_t frames, int32_t hidden, void *workspace, size_t workspace_bytes,
                           int32_t *timeout_flag, void *stream);
int la_gru_layer_bwd(const float *gates, const float *out, const float *dout, const float *w_hh, float *dgi, float *dgh,
                     int32_t batch, int32_t frames, int32_t hidden, void *workspace, size_t workspace_bytes,
                     int32_t *timeout_flag, void *stream);
int la_transpose_pad_f32(const float *in, int64_t ld_in, int32_t rows, int32_t cols, float *out, int64_t ld_out,
                         int32_t out_rows, int32_t out_cols, void *stream);
int la_colsum_f32(const float *in, int64_t ld, int32_t rows, int32_t cols, float *out, void *stream);
int la_mish_f32(const float *x, float *y, int64_t n, void *stream);
int la_mish_bwd_f32(const float *x, const float *dy, float *dx, int64_t n, void *stream);
int la_mask_scale_f32(const float *x, const unsigned char *mask, float scale, float *y, int64_t n, void *stream);

/*
 * LayerNorm folded into the GEMMs on either side of it -- whisper's ResidualAttentionBlock computes
 * x = x + attn(attn_ln(x)); x = x + mlp(mlp_ln(x)) (third-party whisper/model.py; call module/align_model.py:91,101,112,137).
 * In the 16-bit modes, for shapes that run on the 256x256 kernel:
 *   producer  (la_gemm_fused_ln with C2 != NULL, LA_EPI_OUT_F32): the GEMM that writes the f32 residual stream also stores
 *             the same rows rounded to `dtype` into C2 [M][ldc2] -- the RAW operand of the next GEMM;
 *   la_row_stats16 (or ln_part + la_ln_stats_finalize): stats[m] = (mean, 1/sqrt(var + eps)) of those raw rows;
 *   consumer  (ln_stats != NULL): A = raw rows, W = gamma-folded weights W'[n][k] = gamma[k] W[n][k], ln_csum[n] = sum_k W'[n][k],
 *             bias[n] = b[n] + sum_k beta[k] W[n][k]:   LN(x) W^T + b = rstd (x W'^T - mean c) + bias.
 * Replaces the separate LayerNorm pass (read f32, write 16-bit) between them.  LA_EUNSUPPORTED for f32 and for shapes
 * the 256x256 kernel does not take (callers fall back to la_layernorm + la_gemm).
 */
int la_gemm_fused_ln(int32_t dtype, int32_t M, int32_t N, int32_t K, int32_t batch, const void *A, int64_t lda, int64_t strideA,
                     const void *W, void *C, int64_t ldc, int64_t strideC, const float *bias, const float *residual, int64_t ldr,
                     int64_t strideR, int32_t epilogue, void *C2, int64_t ldc2, int64_t strideC2, const float *ln_stats,
                     const float *ln_csum, float *ln_part, void *stream);
/*
 * The residual stream of the 16-bit encoder kept SPLIT (the default of la_encoder_forward wherever the LayerNorm fold applies):
 *   hi [M][ld] `dtype` = x rounded to the operand type -- at the same time the raw A operand of the next folded GEMM,
 *   lo [M][ld] uint8   = the remainder x - hi in steps of ulp(hi) / 254, offset by 128
 * (x to 8 bits below the operand type's last place; 3 + 3 bytes per element through HBM per read-modify-write instead of the
 * 4 + 4 + 2 of an f32 stream with a 16-bit copy).  la_gemm_split: (hi, lo) <- epi(A W^T) + residual, epilogue = LA_EPI_BIAS |
 * LA_EPI_GELU | LA_EPI_RESIDUAL; with LA_EPI_RESIDUAL the residual is `residual` (f32 rows, as la_gemm takes them: the stem's
 * positional embedding) or, when that pointer is NULL, the stream itself, updated in place (x += out-proj, x += mlp:
 * whisper/model.py ResidualAttentionBlock.forward).  ln_part as la_gemm_fused_ln.  LA_EUNSUPPORTED for f32 and for shapes the
 * 256x256 kernel does not take.  la_layernorm_split: la_layernorm over rows of such a stream (ln_post).
 */
int la_gemm_split(int32_t dtype, int32_t M, int32_t N, int32_t K, int32_t batch, const void *A, int64_t lda, int64_t strideA,
                  const void *W, void *hi, void *lo, int64_t ld, int64_t stride, const float *bias, const float *residual,
                  int64_t ldr, int64_t strideR, int32_t epilogue, float *ln_part, void *stream);
int la_layernorm_split(int32_t dtype, const void *hi, const void *lo, int64_t ldx, int32_t M, int32_t d, const float *gamma,
                       const float *beta, void *y, int64_t ldy, int32_t out_dtype, void *stream);
/* producer with ln_part != NULL (N % 64 == 0): also stores, per row and 64-column segment of the 16-bit copy, (mean, sum of
 * squared deviations) into ln_part [N/64][M][2]; la_ln_stats_finalize combines them into stats [M][2] = (mean, rstd) --
 * the same numbers la_row_stats16 computes, without reading the copy back. */
int la_ln_stats_finalize(const float *part, int32_t slots, int32_t M, float eps, float *stats, void *stream);
int la_row_stats16(int32_t dtype, const void *x, int64_t ldx, int32_t M, int32_t d, float eps, float *stats, void *stream);

/* float32 Linear products on the f16 matrix pipe at float32 accuracy ("f16x2"; the fine-tune step's nn.Linear forward and both
 * backward products, train_multitask.py:325-326).  gfx950 multiplies float32 operands at 1/16 of its 16-bit MFMA rate.  A float32
 * matrix, its rows scaled by powers of two (largest magnitude of a row in [2^13, 2^14)), splits exactly into two IEEE-half PLANES
 * (hi = f16(x s), lo = f16(x s - hi): 22 bits), and  A W^T = (sa sw^T) o (A_lo W_hi^T + A_hi W_lo^T + A_hi W_hi^T) + O(2^-22)
 * -- three f16 products accumulated in f32 inside ONE pass of the 256 x 256 kernel over segmented K, the scales applied in its
 * epilogue.  Measured (profiles/r5_kbench_f32emu.txt): 2.5-3.2 x faster than float32 la_gemm on the fine-tune shapes, error against
 * a float64 product SMALLER than float32 la_gemm's own.
 *   la_split_f16x2:    x [rows][cols] f32 (pitch ldx) -> planes [rows][2][kp] f16 (kp >= cols, % 8 == 0; tail columns zero) and
 *                      inv_scale [rows] f32 (1 / s, a power of two).
 *   la_split_f16x2_t:  the same of x^T -- planes_t [cols][2][mp] (mp >= rows, % 16 == 0), inv_scale_t [cols]: the operands of a
 *                      weight gradient dW = dY^T X, whose contraction runs over the rows of dY and X.  Uses library scratch (4 B per column).
 *   la_gemm_f16x2:     C [M][N] f32 (pitch ldc) = epi((A W^T) o sa sw^T); A = planes [M][2][K], W = planes [N][2][K] (K = the padded
 *                      plane length both were split to), epilogue = LA_EPI_BIAS | LA_EPI_GELU (erf) | LA_EPI_RESIDUAL (f32 rows, pitch
 *                      ldr).  slots > 1 cuts K into `slots` equal chunks run as batch slots into library scratch and summed in slot
 *                      order (few tiles, long K: the weight gradients).  Domain: K / slots a multiple of 128 and >= 256, N > 128,
 *                      ceil(M/256) ceil(N/256) slots >= 192 -- else LA_EUNSUPPORTED (the caller keeps float32 la_gemm for small shapes). */
int la_split_f16x2(const float *x, int64_t ldx, int32_t rows, int32_t cols, void *planes, int64_t kp, float *inv_scale, void *stream);
int la_split_f16x2_t(const float *x, int64_t ldx, int32_t rows, int32_t cols, void *planes_t, int64_t mp, float *inv_scale_t, void *stream);
/* the same with an activation applied to the values before the split (act: 0 = none, 1 = exact-erf GELU): the MLP's hidden operand
 * gelu(u) goes from u into its planes without a float32 copy of its own (forward product and weight gradient) */
int la_split_f16x2_act(const float *x, int64_t ldx, int32_t rows, int32_t cols, void *planes, int64_t kp, float *inv_scale, int32_t act, void *stream);
int la_split_f16x2_t_act(const float *x, int64_t ldx, int32_t rows, int32_t cols, void *planes_t, int64_t mp, float *inv_scale_t, int32_t act, void *stream);
/* la_split_f16x2_t_act that also returns colsum[c] = sum_r x[r][c] (NULL: not wanted; act must be 0): the bias gradient sum_r dy next to
 * the weight gradient dy^T x whose operand the split makes, from the same pass over dy (float64 partials per row block, added in order:
 * deterministic, as la_colsum_f32) */
int la_split_f16x2_t_colsum(const float *x, int64_t ldx, int32_t rows, int32_t cols, void *planes_t, int64_t mp, float *inv_scale_t, int32_t act,
                            float *colsum, void *stream);
/* An operand that is split both ways (dy: plain for dx = dy w, transposed for dw = dy^T x; an activation: plain in the forward, transposed
 * for its weight gradient) needs no second pass for the transposed planes' scales: la_split_f16x2_max is la_split_f16x2_act that also
 * leaves the operand's largest magnitude in tmax (2048 words ZEROED by the caller: 64 are used, one per 128-byte line, filled with atomicMax), and la_split_f16x2_t_tmax with
 * that tmax gives the transposed planes ONE power-of-two scale for the whole operand (tmax NULL = la_split_f16x2_t_colsum: a scale per
 * column).  Entries more than 2^17 below the operand's maximum lose relative, never absolute (2^-39 of the maximum), precision. */
int la_split_f16x2_max(const float *x, int64_t ldx, int32_t rows, int32_t cols, void *planes, int64_t kp, float *inv_scale, int32_t act,
                       uint32_t *tmax, void *stream);
int la_split_f16x2_t_tmax(const float *x, int64_t ldx, int32_t rows, int32_t cols, void *planes_t, int64_t mp, float *inv_scale_t, int32_t act,
                          float *colsum, const uint32_t *tmax, void *stream);
int la_gemm_f16x2(int32_t M, int32_t N, int32_t K, int32_t slots, const void *A, const float *sa, const void *W, const float *sw,
                  float *C, int64_t ldc, const float *bias, const float *residual, int64_t ldr, int32_t epilogue, void *stream);
/* la_gemm_f16x2 on the 128 x 128 tile, for the products outside the 256 x 256 kernel's domain (few rows: float32 inference at 1-8 clips,
 * option x2_small).  Same operands, epilogue and `slots` meaning; where both kernels accept a shape with slots = 1 the results are
 * bit-identical (same f16 MFMA sequence per output element, same epilogue arithmetic).  Domain: M, N >= 1, K / slots a multiple of 32, at
 * most 64 slots -- else LA_EUNSUPPORTED.  slots = 0: la_gemm_f16x2_small_slots(M, N, K), which fills about 512 workgroups (two per CU)
 * and keeps at least 256 of K per slot. */
int la_gemm_f16x2_small(int32_t M, int32_t N, int32_t K, int32_t slots, const void *A, const float *sa, const void *W, const float *sw,
                        float *C, int64_t ldc, const float *bias, const float *residual, int64_t ldr, int32_t epilogue, void *stream);
int la_gemm_f16x2_small_slots(int32_t M, int32_t N, int32_t K);
/* Which kernel takes a product: pure host queries (no device call) for callers that route products themselves, so that they ask the
 * library's rule instead of restating it.
 *   la_gemm_f16x2_domain:  1 where (M, N, K, slots) lies in la_gemm_f16x2's domain (the test that entry makes), else 0.
 *   la_gemm_f16x2_slots:   the split-K slots that bring an M x N product with few 256 x 256 tiles up to that domain (1 = none needed).
 *   la_gemm_fills_chip:    1 where a 16-bit la_gemm of M x N x batch runs on the 256 x 256 kernel (option gemm_tile = 0): N > 128 and
 *                          enough 256 x 256 tiles x batch to fill the chip. */
int la_gemm_f16x2_domain(int32_t M, int32_t N, int32_t K, int32_t slots);
int la_gemm_f16x2_slots(int32_t M, int32_t N);
int la_gemm_fills_chip(int32_t M, int32_t N, int32_t batch);
/* la_layernorm (eps 1e-5, statistics in float32 over the row) whose result leaves as the f16x2 planes of the next Linear's operand instead of
 * as float32 rows: planes [rows][2][kp] + inv_scale [rows] as la_split_f16x2 would make them from LN(x) gamma + beta (float32 inference on the
 * f16x2 products: module/align_model.py:72-123 is float32 throughout).  d % 4 == 0, d <= 4096. */
int la_layernorm_f16x2(const float *x, int64_t ldx, int32_t rows, int32_t d, const float *gamma, const float *beta, void *planes, int64_t kp,
                       float *inv_scale, void *stream);

/* Backward-pass building blocks of the Whisper encoder (float32): la_gemm with a row pitch for W and per-batch strides
 * (attention gradients batch over heads inside the packed [T][3d] projections), batched zero-padded transposes, exact-erf
 * GELU forward / backward, LayerNorm backward (dx and dy*xhat, whose column sum is dgamma), row softmax forward /
 * backward on materialised score tiles, the overlap-add of the k=3 convolution gradients, elementwise add. */
int la_gemm_ex(int32_t dtype, int32_t M, int32_t N, int32_t K, int32_t batch, const void *A, int64_t lda, int64_t strideA,
               const void *W, int64_t ldw, int64_t strideW, void *C, int64_t ldc, int64_t strideC, const float *bias,
               int32_t epilogue, void *stream);
int la_transpose_pad_batched_f32(const float *in, int64_t ld_in, int64_t batch_stride_in, int32_t rows, int32_t cols,
                                 float *out, int64_t ld_out, int64_t batch_stride_out, int32_t out_rows, int32_t out_cols,
                                 int32_t batch, void *stream);
int la_gelu_f32(const float *x, float *y, int64_t n, void *stream);
int la_gelu_bwd_f32(const float *x, const float *dy, float *dx, int64_t n, void *stream);
int la_add_f32(const float *a, const float *b, float *y, int64_t n, void *stream);
int la_scale_f32(const float *x, float alpha, float *y, int64_t n, void *stream);
int la_layernorm_bwd_f32(const float *x, const float *dy, const float *gamma, int32_t M, int32_t d, float *dx, float *dy_xhat,
                         void *stream);
/* la_layernorm_bwd_f32 together with the parameter gradients dgamma [d] = sum_r dy xhat and dbeta [d] = sum_r dy: one pass over x and dy for
 * d = 256 ... 2048 in steps of 256 with 16-byte aligned x, dy, gamma, dx, residual (rows in registers; float64 partials per block of 4 x rpw rows
 * added in order, rpw = rows per wave, 32 down to 2, chosen from M so that about 512 blocks exist); other widths or alignments run
 * la_layernorm_bwd_f32 into `scratch` (M x d floats, required then, may be NULL otherwise) and two la_colsum_f32.  residual [M][d] (or
 * NULL): added to dx -- the gradient that reaches the block's input past it (pre-norm residual connection). */
int la_layernorm_bwd_sums_f32(const float *x, const float *dy, const float *gamma, const float *residual, int32_t M, int32_t d, float *dx,
                              float *dgamma, float *dbeta, float *scratch, void *stream);
/* In-place softmax over the first `cols` columns of each row; the pad columns cols .. ld - 1 of every row are set to 0.
 * causal_q_len > 0: row r is query (r mod causal_q_len) and sees keys 0 .. (r mod causal_q_len) + cols - causal_q_len; masked entries become
 * exact zeros.  With cols < causal_q_len a query for which that range is empty is given key 0 alone (probability 1 there), never an empty row. */
int la_softmax_rows_f32(float *s, int64_t ld, int64_t rows, int32_t cols, int32_t causal_q_len, void *stream);
int la_softmax_bwd_rows_f32(const float *p, float *dp, int64_t ld, int64_t rows, int32_t cols, void *stream);
/* Fused float32 attention backward, head_dim 64 (the gradient of whisper/model.py MultiHeadAttention.qkv_attention, reached from
 * train_multitask.py:325-326): q [batch*q_len][ld_q] (pre-scaled by head_dim^-0.5, as la_attention takes it), k / v
 * [batch*kv_len][ld_kv], o = the forward output and dout its gradient [batch*q_len][ld_o / ld_do]; head h owns columns
 * 64 h .. 64 h + 63 of every operand.  Writes dq [batch*q_len][ld_dq] (w.r.t. the pre-scaled q) and dk / dv [batch*kv_len][ld_dkv].
 * Nothing of size q_len x kv_len is materialised: scores are recomputed per 64 x 64 tile (three launches: row statistics,
 * a key-block sweep for dk / dv, a query-block sweep for dq).  workspace: la_attention_bwd_workspace_bytes (2 floats per
 * query row and head).  lse: the forward's row statistic (la_attention_lse_f32) or NULL.  causal != 0: key j is visible to queries i >= j (q_len == kv_len). */
int la_attention_bwd_workspace_bytes(int32_t batch, int32_t q_len, int32_t n_head, size_t *bytes);
int la_attention_bwd_f32(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, const float *o, int64_t ld_o,
                         const float *dout, int64_t ld_do, float *dq, int64_t ld_dq, float *dk, float *dv, int64_t ld_dkv,
                         int32_t batch, int32_t q_len, int32_t kv_len, int32_t n_head, int32_t causal, const float *lse,
                         void *workspace, size_t workspace_bytes, void *stream);
/* The statistics launch of la_attention_bwd_f32 alone (lse unless handed in, D = sum dO o O per query row). */
int la_attention_bwd_stats_f32(const float *q, int64_t ld_q, const float *k, int64_t ld_kv, const float *o, int64_t ld_o, const float *dout,
                               int64_t ld_do, int32_t batch, int32_t q_len, int32_t kv_len, int32_t n_head, int32_t causal,
                               const float *lse_in, float *lse, float *dvec, void *stream);
/* The float32 training forward: la_attention_ex(LA_F32, ...) that also writes lse [batch][n_head][q_len] = log sum_j exp(s_ij);
 * handed to la_attention_bwd_f32 (`lse`; NULL there = recomputed by one more sweep over the scores). */
int la_attention_lse_f32(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, float *out, int64_t ld_out,
                         int32_t batch, int32_t q_len, int32_t kv_len, int32_t n_head, int32_t causal, float *lse, void *stream);
/* la_attention_lse_f32 with both products on the f16 matrix pipe at float32 accuracy (the f16x2 scheme of la_gemm_f16x2: operands split
 * into half planes with one power-of-two scale per (clip, head), three 32x32x16 f16 MFMAs per product, float32 accumulate and softmax;
 * csrc/la_attention_f16x2.hip).  Same arguments and results; workspace (256-byte aligned) of la_attention_f16x2_workspace_bytes bytes
 * holds the planes of q, k, v. */
int la_attention_f16x2_workspace_bytes(int32_t batch, int32_t q_len, int32_t kv_len, int32_t n_head, size_t *bytes);
int la_attention_lse_f16x2(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, float *out, int64_t ld_out,
                           int32_t batch, int32_t q_len, int32_t kv_len, int32_t n_head, int32_t causal, float *lse, void *workspace,
                           size_t workspace_bytes, void *stream);
/* la_attention_bwd_f32 with its seven products on the f16 matrix pipe at float32 accuracy (key sweep and query sweep in the
 * register-resident form of la_attention_lse_f16x2; q, k, v, dout split into half planes per clip and head; P split with 2^13, dS with a
 * scale from the bound 2 |dO_i| |v_j|).  Same arguments and results; lse may be NULL (recomputed); workspace (256-byte aligned) of
 * la_attention_bwd_f16x2_workspace_bytes bytes. */
int la_attention_bwd_f16x2_workspace_bytes(int32_t batch, int32_t q_len, int32_t kv_len, int32_t n_head, size_t *bytes);
int la_attention_bwd_f16x2(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, const float *o, int64_t ld_o,
                           const float *dout, int64_t ld_do, float *dq, int64_t ld_dq, float *dk, float *dv, int64_t ld_dkv,
                           int32_t batch, int32_t q_len, int32_t kv_len, int32_t n_head, int32_t causal, const float *lse,
                           void *workspace, size_t workspace_bytes, void *stream);
/* Text-decoder training pieces (whisper/model.py TextDecoder; train_multitask.py:285,308 decoder cross-entropy):
 * gradient of token + learned positional embedding (dtok accumulates, dpos [n][d] is written), and
 * F.cross_entropy(logits [rows][vocab], target, ignore_index=-100, 'mean'): loss2[0] = loss, loss2[1] = 1/count;
 * row_ws holds 2*rows floats; dlogits (optional) = scale * dloss/dlogits. */
int la_embed_tokens_bwd_f32(const float *dx, const int64_t *tokens, int32_t batch, int32_t n, int32_t d, int32_t n_vocab, float *dtok,
                            float *dpos, void *stream);      /* ids clamped to [0, n_vocab) like la_embed_tokens */
int la_cross_entropy_f32(const float *logits, int64_t ld, int32_t rows, int32_t vocab, const int64_t *target, float scale,
                         float *loss2, float *row_ws, float *dlogits, int64_t ld_d, void *stream);
int la_col2im3_f32(const float *dcols, int32_t batch, int32_t t_out, int32_t stride, int32_t channels, float *out,
                   int32_t rows_out, void *stream);

/*
 * Polyphase FIR resampling (audio front end, utils/audio.py:3-20: librosa.load(file, sr=16000)):
 * y[n] = sum_k h[(n + skip)*down - k*up] * x[k], n < n_out.  h is the centred low-pass (host-built Kaiser-windowed sinc,
 * gain `up`, zero pre-padded so that `skip` whole output samples are dropped), as in scipy.signal.resample_poly.
 */
int la_resample_poly_f32(const float *x, int64_t n_in, const float *h, int64_t h_len, int32_t up, int32_t down,
                         int64_t skip, float *y, int64_t n_out, void *stream);

/* elementwise helpers used by the host-side plumbing */
int la_cast_f32_to_bf16(const float *x, void *y, int64_t n, void *stream);
int la_cast_bf16_to_f32(const void *x, float *y, int64_t n, void *stream);

/* ------------------------------------------------------------------------- */
/* model-level entry points: one call per stage of the hot path                */
/* ------------------------------------------------------------------------- */
/*
 * Packed weights (device pointers; layouts = lyricalignment_amd/engine.py pack_encoder / pack_head, which build these
 * structs from an openai-whisper AudioEncoder state_dict and the reference's RNN state_dict):
 *   matrices keep nn.Linear's [out][in] layout in the compute dtype; vectors are f32;
 *   wqkv [3d][d] = rows of query (pre-scaled by head_dim^-0.5; by head_dim^-0.5 log2(e) when la_encoder_weights.dtype carries
 *   LA_Q_LOG2), key, value; bqkv its bias (key part zero, query part scaled like the rows);
 *   conv1_w [d][3][128] (tap-major, mel channels zero-padded 80 -> 128), conv2_w [d][3][d];
 *   *_ln (16-bit modes, optional): the LayerNorm-folded forms la_gemm_fused_ln consumes -- W' = gamma o W rounded to the
 *   compute dtype, c[n] = sum_k W'[n][k], b' = b + W beta; NULL = always the separate LayerNorm pass.
 */
typedef struct la_encoder_block {
    const float *ln1_g, *ln1_b;
    const void *wqkv; const float *bqkv;
    const void *wo; const float *bo;
    const float *ln2_g, *ln2_b;
    const void *w1; const float *b1;
    const void *w2; const float *b2;
    const void *wqkv_ln; const float *cqkv, *bqkv_ln;
    const void *w1_ln; const float *c1, *b1_ln;
    /* float32 mode (ABI 2): the four weight matrices also as f16x2 planes [N][2][K] (la_split_f16x2 of wqkv, wo, w1, w2 with kp = K) and
     * their per-row inverse scales [N] -- all eight given: the block's Linear layers, LayerNorms and attention run on the f16 matrix pipe
     * at float32 accuracy (la_gemm_f16x2, la_layernorm_f16x2, la_attention_lse_f16x2) where the batch brings every product into that
     * kernel's domain; NULL: the float32-MFMA kernels.  Ignored in the 16-bit modes. */
    const void *wqkv_x2; const float *wqkv_x2s;
    const void *wo_x2; const float *wo_x2s;
    const void *w1_x2; const float *w1_x2s;
    const void *w2_x2; const float *w2_x2s;
} la_encoder_block;

typedef struct la_encoder_weights {
    int32_t dtype, d, n_head, n_layer, n_mels;
    const void *conv1_w; const float *conv1_b;
    const void *conv2_w; const float *conv2_b;
    const float *pos;                     /* [1500][d] sinusoids                                   */
    const float *lnp_g, *lnp_b;           /* ln_post                                               */
    const la_encoder_block *blocks;       /* HOST array of n_layer entries                         */
} la_encoder_weights;

/*
 * whisper_model.embed_audio(mel) (module/align_model.py:91,101,112,137 = whisper AudioEncoder.forward): mel [batch][n_mels][3000]
 * f32 -> out [batch*1500][d] rows (`out_dtype`, row pitch ld_out) = ln_post(blocks(conv stem(mel) + positional embedding)).
 * Enqueues the whole kernel sequence on `stream` out of `workspace` (256-byte aligned, la_encoder_workspace_bytes; about
 * 58 MB per clip for Whisper-medium in bf16).  No allocation, no synchronisation.
 */
int la_encoder_workspace_bytes(const la_encoder_weights *w, int32_t batch, size_t *bytes);
int la_encoder_forward(const la_encoder_weights *w, const float *mel, int64_t mel_batch_stride, int64_t mel_row_stride,
                       int32_t batch, void *out, int64_t ld_out, int32_t out_dtype, void *workspace, size_t workspace_bytes,
                       void *stream);

typedef struct la_head_weights {
    int32_t dtype, hidden, in_dim, vocab, n_layers;   /* n_layers = 2, bidirectional (module/align_model.py:23-28) */
    const void *w_ih[2]; const float *b_ih[2];        /* per layer [6H][in] (forward rows, then reverse), [6H]     */
    const void *w_hh[2]; const float *b_hh[2];        /* per layer [2][3H][H], [2][3H]                              */
    const void *w_fc; const float *b_fc;              /* [V][2H], [V]                                               */
    /* float32 mode (ABI 2): the input projections and the output Linear also as f16x2 planes ([6H][2][in], [V][2][2H]; la_split_f16x2 with
     * kp = the matrix's own K) + per-row inverse scales -- given: those products and the recurrence's W_hh h run on the f16 matrix pipe at
     * float32 accuracy; NULL: the float32-MFMA kernels.  Ignored in the 16-bit modes. */
    const void *w_ih_x2[2]; const float *w_ih_x2s[2];
    const void *w_fc_x2; const float *w_fc_x2s;
} la_head_weights;

/*
 * align_rnn(embed) + perform_viterbi(_ctc) (module/align_model.py:35-38; utils/alignment.py:13-71,121-188) without the
 * logits: feats rows [.][ld_feats] (compute dtype), clip b at rows b*clip_stride_rows .. +frames -> 2 x {input-projection
 * GEMM, persistent BiGRU recurrence} -> Mish -> fused Linear + emission prep -> batched DP -> onset / offset frames
 * (same outputs as la_viterbi_batch).  emissions_out (optional) [batch][frames][max_labels+1] f32 receives the compact
 * emissions.  More clips than one launch set of the recurrence takes (256; 144 in float32 at hidden 384) run as
 * consecutive slices inside this call.  `timeout_flag`: see la_gru_layer.
 */
int la_align_head_workspace_bytes(const la_head_weights *w, int32_t batch, int32_t frames, int32_t max_labels, size_t *bytes);
int la_align_head_forward(const la_head_weights *w, const void *feats, int64_t ld_feats, int64_t clip_stride_rows,
                          int32_t batch, int32_t frames, int32_t variant, const int32_t *labels, int32_t labels_stride,
                          const int32_t *n_labels, int32_t max_labels, int32_t *onset, int32_t *offset, int32_t out_stride,
                          double *final_score, int32_t *status, float *emissions_out, void *workspace, size_t workspace_bytes,
                          int32_t *timeout_flag, void *stream);
/*
 * Clips of different lengths in one call (an addition; the reference runs one frame count over a whole batch, which
 * la_align_head_forward reproduces): n_frames [batch] (device int32), n_frames[b] <= frames = the maximum.  The input projections
 * and the fused Linear + emission prep run over `frames` rows per clip, the two recurrences (la_gru_layer_ragged) and the DP take
 * the lengths: clip b's onset / offset / final_score / status are those of la_align_head_forward for that clip alone with
 * frames = n_frames[b] (n_frames[b] = 0: status LA_EINVAL for that clip only).  emissions_out rows t >= n_frames[b] are
 * unspecified.  Slices of clips (see above) get their own part of n_frames.  Workspace: la_align_head_workspace_bytes.
 */
int la_align_head_forward_ragged(const la_head_weights *w, const void *feats, int64_t ld_feats, int64_t clip_stride_rows,
                                 int32_t batch, int32_t frames, const int32_t *n_frames, int32_t variant, const int32_t *labels,
                                 int32_t labels_stride, const int32_t *n_labels, int32_t max_labels, int32_t *onset, int32_t *offset,
                                 int32_t out_stride, double *final_score, int32_t *status, float *emissions_out, void *workspace,
                                 size_t workspace_bytes, int32_t *timeout_flag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LYRICALIGN_H */
