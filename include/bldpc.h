/*
 * bldpc.h -- C ABI of the MI355X-native binary QC-LDPC flooding min-sum decoder.
 *
 * This is the drop-in boundary for the reference's binary hot path
 * (gsw4869/CUDA_LDPC, directory bldpc_实习/).  Every entry point names the
 * reference interface it replaces.  Plain pointers and sizes only; no C++ or
 * torch types.  All functions return BLDPC_OK (0) or a negative error code and
 * never call exit() (the reference printf+exit(0)s on every failure,
 * LDPC_Decoder.cu:39-44); bldpc_last_error() returns a message for the calling
 * thread.
 *
 * Data layouts are the reference's:
 *   Channel_Out  float  [N][F]   frame-fastest, device        (LDPC_Decoder.cu:23, Simulation.cu:74)
 *   D            int32  [N+1][F] frame-fastest; row N = per-frame flag
 *                                "first `length` decoded bits are all zero"    (LDPC_Decoder.cu:134-147)
 *   Address_Variablenode int32 [N][Wv]: Memory_RQ slot (m*Wc+p) of each edge   (Simulation.cu:363-387)
 *   Weight_Checknode [J+1], Weight_Variablenode [L+1]: block weights, last = max (Simulation.cu:321-340)
 * with N = L*Z, M = J*Z, Wc/Wv the maximum block-row / block-column weights.
 * J, L, Z, the batch size F, maxIT and msgLen are compile-time macros in the
 * reference (define.cuh:20-61); here they are run-time arguments.
 */
#ifndef CUDA_LDPC_AMD_BLDPC_H
#define CUDA_LDPC_AMD_BLDPC_H

#ifdef __cplusplus
extern "C" {
#endif

#define BLDPC_OK 0
#define BLDPC_EINVAL (-1)       /* bad argument / inconsistent shapes            */
#define BLDPC_ENOMEM (-2)       /* host or device allocation failed              */
#define BLDPC_EHIP (-3)         /* a HIP runtime call failed                     */
#define BLDPC_EIO (-4)          /* file could not be opened / parsed             */
#define BLDPC_EUNSUPPORTED (-5) /* requested kernel cannot run this code         */

/* early-exit modes of bldpc_decode */
#define BLDPC_EXIT_FIXED 0        /* run exactly max_iter iterations (benchmark mode)                       */
#define BLDPC_EXIT_BATCH_GLOBAL 1 /* reference rule: stop after the first iteration at which ALL F frames   */
                                  /* have their flag set (LDPC_Decoder.cu:150-153)                          */
#define BLDPC_EXIT_PER_FRAME 2    /* the same rule applied to every frame on its own (what the reference does with  */
                                  /* Num_Frames_OneTime = 1): bldpc_decode_per_frame only                           */

/* kernel selection */
#define BLDPC_KERNEL_AUTO 0   /* QC_LDS when the code has QC structure and fits LDS, else TABLE */
#define BLDPC_KERNEL_TABLE 1  /* generic address-table kernels, messages resident in HBM; any table      */
#define BLDPC_KERNEL_QC_LDS 2 /* fused QC kernels, all iterations on-chip: messages in LDS, or (larger codes)  *
                               * compressed check states in LDS / in registers with the a-posteriori values in LDS */

typedef struct bldpc_code bldpc_code; /* opaque: device-resident code tables + cached workspace.  A code object owns
                                        * its scratch buffers: use it from one host thread / one stream at a time (create
                                        * one object per concurrent stream, like a BLAS handle); different objects are
                                        * independent. */

/* -- graph builders ------------------------------------------------------- */

/* Replaces Get_H (Simulation.cu:292-354) without its hard-coded file name and
 * weight-range exits: reads J*L shifts (-1 = zero block) and fills the block
 * weights. H[J*L], Weight_Checknode[J+1], Weight_Variablenode[L+1]: host. */
int bldpc_read_blockh(const char *path, int J, int L, int *H, int *Weight_Checknode, int *Weight_Variablenode);

/* Replaces Transform_H (Simulation.cu:363-387). as_written = 0 builds the
 * intended circulant (column c of a block with shift s meets row (c-s) mod Z);
 * as_written = 1 reproduces the reference expression at :380 literally (its
 * else-branch maps columns c < s to row c).
 * Address_Variablenode[N*Wv]: host, unused entries -1 (main.cu:94). */
int bldpc_transform_h(const int *H, int J, int L, int Z, const int *Weight_Checknode, const int *Weight_Variablenode,
                      int *Address_Variablenode, int as_written);

/* -- code objects --------------------------------------------------------- */

/* Build a decoder for the QC code with block shifts H[J*L] (host).  Uploads the
 * circulant description for the fused LDS kernel AND the equivalent (correct)
 * address table for the generic kernels. */
int bldpc_code_create_qc(int J, int L, int Z, const int *H, bldpc_code **code);

/* Build a decoder from an arbitrary host address table with the reference's
 * semantics (what main.cu:98 uploads), including the as-written table whose
 * colliding slots make the reference's own output order-dependent; here the
 * order is defined as ascending variable-node index within each iteration
 * (the order of a sequential emulation of the reference launch), enforced by
 * level-scheduled launches.  Only BLDPC_KERNEL_TABLE can run such a code. */
int bldpc_code_create_table(int J, int L, int Z, const int *Weight_Checknode, const int *Weight_Variablenode,
                            const int *Address_Variablenode, bldpc_code **code);

int bldpc_code_destroy(bldpc_code *code);

/* dims[0..7] = N, M, K (= N-M), Wc, Wv, nnz blocks, VN levels (1 = conflict-free table),
 *              frames per workgroup of the QC_LDS kernel (0 = code does not fit LDS / no QC structure) */
int bldpc_code_dims(const bldpc_code *code, int dims[8]);

/* -- decode ---------------------------------------------------------------- */

/* Replaces LDPC_Decoder_GPU (LDPC_Decoder.cuh:5, LDPC_Decoder.cu:23-164).
 *   Channel_Out   device float [N][F]                         (in)
 *   F             frames in this call (reference: Num_Frames_OneTime)
 *   max_iter      reference: maxIT (define.cuh:35)
 *   length        bits examined by the termination test; reference: msgLen
 *                 (Message_CW == 0) or CW_Len; pass 0 for K = N - M
 *   exit_mode     BLDPC_EXIT_*
 *   kernel        BLDPC_KERNEL_*
 *   D             device int32 [N+1][F]                       (out) hard bits of the last executed
 *                 iteration + flag row, as the reference leaves them in its host D
 *   app           optional device float [N][F]                (out) a-posteriori sums (Add_result,
 *                 LDPC_Decoder.cu:201-204) of the last executed iteration; NULL to skip
 *   flag_hist     optional device uint64 [F]                  (out) bit (it-1) = flag of frame after
 *                 iteration it, it <= 64; NULL to skip
 *   iteraTime     host int                                    (out) iterations executed
 *                 (LDPC->iteraTime, batch-global like the reference)
 *   stream        hipStream_t (NULL = default stream).  The call is asynchronous in
 *                 BLDPC_EXIT_FIXED mode; BATCH_GLOBAL synchronises the stream (it reads flags).
 * No per-call allocation: scratch lives in the code object and grows on demand. */
int bldpc_decode(bldpc_code *code, const float *Channel_Out, int F, int max_iter, int length, int exit_mode, int kernel,
                 int *D, float *app, unsigned long long *flag_hist, int *iteraTime, void *stream);

/* Per-frame termination: frame f stops after the first iteration at which ITS flag is set -- the
 * reference's rule (LDPC_Decoder.cu:134-153) as it acts on a batch of one frame -- and column f of D (and of app) holds
 * the outputs of that iteration, exactly what LDPC_Decoder_GPU returns for that frame with Num_Frames_OneTime = 1;
 * a frame whose flag never comes up runs max_iter iterations.  Nothing is recomputed and nothing waits for the slowest
 * frame of the batch: on the fused kernels a workgroup leaves when its own (1-2) frames have stopped, so the cost of a
 * batch follows the MEAN iteration count (BER sweeps at operating SNR: several times the fixed-iteration rate).
 *   iters   device int32 [F]  (out) iterations executed by each frame (the reference's iteraTime of that frame)
 * Other arguments as bldpc_decode.  Asynchronous on `stream` with the fused kernels; the table kernels read one
 * counter per iteration, as for BATCH_GLOBAL. */
int bldpc_decode_per_frame(bldpc_code *code, const float *Channel_Out, int F, int max_iter, int length, int kernel, int *D,
                           float *app, int *iters, void *stream);

/* Device-side Statistic (Simulation.cu:245-262) over one decoded batch against
 * the all-zero codeword (PN_Message 0, define.cuh:26) or CodeWord (device int32
 * [N][F], may be NULL = all-zero).  counters: device int64[5], ACCUMULATED:
 *   [0] num_Error_Frames [1] num_Error_Bits [2] Total_Iteration (+= iteraTime per frame)
 *   [3] num_False_Frames [4] num_Alarm_Frames.   num_Frames is the caller's (+= F). */
int bldpc_statistic(const bldpc_code *code, const int *D, const int *CodeWord, int F, int length, int iteraTime,
                    long long *counters, void *stream);

/* The same with one iteration count per frame (bldpc_decode_per_frame): Total_Iteration += iters[f]. */
int bldpc_statistic_per_frame(const bldpc_code *code, const int *D, const int *CodeWord, int F, int length, const int *iters,
                              long long *counters, void *stream);

/* bldpc_decode (iters == NULL; FIXED or BATCH_GLOBAL exit) or bldpc_decode_per_frame (iters != NULL, exit_mode PER_FRAME)
 * followed by bldpc_statistic / bldpc_statistic_per_frame against the all-zero codeword, the pair of calls of the
 * reference's Simulation_GPU loop (Simulation.cu:143-145): D, *iteraTime / iters and the accumulated counters are the same
 * as from the two calls.  With the fused kernels and a single launch (FIXED, PER_FRAME) the message-bit errors are counted
 * from the packed hard bits while D is written, which saves the statistics pass over D. */
int bldpc_decode_statistic(bldpc_code *code, const float *Channel_Out, int F, int max_iter, int length, int exit_mode, int kernel,
                           int *D, int *iters, long long *counters, int *iteraTime, void *stream);

/* Host input generator, bit-identical to the reference's (the "identical AWGN inputs" of the parity
 * contract): AWGNChannel_CPU + RandomModule (LDPC_Encoder.cu:25-56).  seed[3] is advanced in place
 * (AWGNChannel.seed, struct.cuh:13), sigma as main.cu:120-127 computes it (bldpc_sigma below).
 * Channel_Out: HOST float [N][F], frame-outer / bit-inner draw order; CodeWord: host int32 [N][F] or
 * NULL for the all-zero codeword. */
int bldpc_awgn_channel_host(int seed[3], float sigma, float *Channel_Out, const int *CodeWord, int N, int F);

/* Device-side input generator: the same channel on the GPU.  The three LCGs of RandomModule are
 * advanced by modular exponentiation (seed * a^k mod m), so thread (f, n) produces exactly the draws u1, u2 the
 * serial host loop would have produced for that sample (integer and IEEE float arithmetic only: bit-identical);
 * the Box-Muller transform then uses the device math library, whose logf / sin differ from glibc's in the last
 * ulp on a small fraction of arguments -- samples are identical or 1 ulp apart, statistically the same channel.
 * Channel_Out: DEVICE float [N][F]; CodeWord: device int32 [N][F] or NULL.  seed[3] (host) is advanced by the
 * whole batch exactly like bldpc_awgn_channel_host. */
int bldpc_awgn_channel_device(int seed[3], float sigma, float *Channel_Out, const int *CodeWord, int N, int F, void *stream);

/* -- encoder and syndrome (PN_Message 1, define.cuh:26) ------------------- */

/* The reference simulates only the all-zero codeword: its PN_Message 1 branch (Simulation.cu:107) is empty.  These
 * entry points encode real messages for codes made by bldpc_code_create_qc (H convention of the decoders: column c of a
 * block with shift s meets row (c - s) mod Z); codes made by bldpc_code_create_table return BLDPC_EUNSUPPORTED.
 *
 * Generator: Gauss-Jordan over GF(2) on the dense H, pivot columns searched from the right (N-1 down to 0).  The pivot
 * columns are the parity positions, the other K' = N - rank(H) columns the information set info_pos[K'] (ascending);
 * information bit k of a message goes to codeword position info_pos[k].  Parity row r belongs to the r-th parity
 * position in ascending order, and that codeword bit is the XOR of the information bits j for which bit j of row r of
 * P is set: P is uint64 [rank][ceil(K'/64)], bit j in word j/64 at bit j%64.  For codes whose last M columns are
 * invertible, info_pos = 0 .. K-1 with K = N - M. */

/* Host only (no device needed): the generator of the QC code with block shifts H[J*L].  Sizes come back in *K_info
 * and *rank; info_pos (int [K']) and P (rank * ceil(K'/64) words) are filled when not NULL, so a call with both NULL
 * returns the sizes.  Dense elimination on up to 16 threads: a few seconds for N = 38 400, well under one below. */
int bldpc_generator_host(int J, int L, int Z, const int *H, int *K_info, int *rank, int *info_pos, unsigned long long *P);

/* K', rank and (when not NULL) info_pos[K'] of the code's generator.  The generator is built on the first call of this
 * function, bldpc_encode or bldpc_encode_random on the code object, and kept with it. */
int bldpc_encoder_info(bldpc_code *code, int *K_info, int *rank, int *info_pos);

/* Systematic encoding of F messages on the device.
 *   msg       device int32 [K'][F]  (in)  frame-fastest; only bit 0 of each entry is read
 *   CodeWord  device int32 [N][F]   (out) frame-fastest, as everywhere in this ABI: 0/1 per bit, H * c = 0,
 *             CodeWord[info_pos[k]][f] = msg[k][f] & 1
 * Asynchronous on `stream` (after the generator exists).  K' is limited to 20 480 (the slices of 64 frames fill the LDS
 * of one CU); every shipped matrix fits. */
int bldpc_encode(bldpc_code *code, const int *msg, int F, int *CodeWord, void *stream);

/* The same with messages generated on the device by a counter-based rule, so that any frame can be drawn on its own
 * (a sharded sweep gets the same codewords at any world size).  For global frame g = first_frame + f, f < F:
 *     bit k of the message = (splitmix64(seed + g * ceil(K'/64) + k / 64) >> (k % 64)) & 1     (uint64 arithmetic, wrapping)
 * with splitmix64(x) the first output of SplitMix64 seeded with x:
 *     z = x + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *     return z ^ (z >> 31);
 *   first_frame >= 0;  msg  optional device int32 [K'][F] (out): the messages, NULL to skip;  CodeWord as bldpc_encode. */
int bldpc_encode_random(bldpc_code *code, unsigned long long seed, long long first_frame, int F, int *msg, int *CodeWord,
                        void *stream);

/* Syndrome check of F hard-decision words: flag[f] = 1 iff H * d_f = 0 over bit 0 of D[0..N-1][f], and unsat[f] = the
 * number of unsatisfied checks.
 *   D      device int32 [N][F] (or the [N+1][F] output of bldpc_decode)
 *   flag   device int32 [F]: may be row N of D (D + N*F), which then takes the meaning "valid codeword" in place of the
 *          decoders' "first `length` bits are zero"; bldpc_statistic against the sent CodeWord then counts a frame as an
 *          error frame when it has bit errors or a failed syndrome, and num_False_Frames = undetected errors
 *   unsat  device int32 [F] or NULL
 * Asynchronous on `stream`. */
int bldpc_syndrome(const bldpc_code *code, const int *D, int F, int *flag, int *unsat, void *stream);

/* -- row-layered normalised min-sum (not in the reference, which only floods) ------------------------------------ */

/* stop rules of bldpc_decode_layered: what the flag row of D means and what the per-frame exit tests */
#define BLDPC_STOP_PREFIX 0   /* the first `length` hard bits are all zero (the rule of bldpc_decode; all-zero codeword only) */
#define BLDPC_STOP_SYNDROME 1 /* H * d = 0, the rule of bldpc_syndrome: valid for any sent codeword                        */

/* Layered ("turbo decoding message passing") normalised min-sum for codes made by bldpc_code_create_qc: every block row
 * of the QC matrix is a layer whose Z checks touch disjoint variables.  Semantics, IEEE fp32 without fused multiply-add:
 *
 *   state per frame: S[N] = Channel_Out (a-posteriori values), R = +0.0f per edge.
 *   one iteration visits the layers j = 0 .. J-1 in order; in layer j, for every t in 0 .. Z-1 (independent of each other),
 *   with the non-zero blocks of block row j in ascending block column l_0 < ... < l_{w-1}, shifts s_i,
 *   v_i = l_i*Z + (t + s_i) mod Z:
 *     1. Q_i = S[v_i] - R_i
 *     2. sg_i = sign BIT of Q_i;  P = XOR of all sg_i;  a_i = |Q_i|;  m1 <= m2 the two smallest a_i with multiplicity;
 *        first = lowest i with a_i == m1
 *     3. mag_i = alpha * (i == first ? m2 : m1)   (one fp32 multiplication; alpha = 1.0f is plain min-sum)
 *        R_i' = (P xor sg_i) ? -mag_i : +mag_i
 *     4. S[v_i] = Q_i + R_i';  R_i' replaces R_i
 *   after each iteration the hard bits are d[v] = S[v] < 0 and the frame's flag is, by stop_rule, BLDPC_STOP_PREFIX
 *   (length = 0 means K = N - M) or BLDPC_STOP_SYNDROME.
 *
 *   exit_mode  BLDPC_EXIT_FIXED: exactly max_iter iterations.  BLDPC_EXIT_PER_FRAME: frame f stops after the first iteration
 *              at which its flag is set (else after max_iter); column f of D and app hold that iteration's outputs and
 *              iters[f] its number -- what a fixed run of iters[f] iterations on that frame alone returns.
 *              BLDPC_EXIT_BATCH_GLOBAL is a property of the reference's flooding driver and is refused (BLDPC_EINVAL).
 *   alpha      normalisation factor in (0, 1]
 *   D          device int32 [N+1][F] (out): hard bits, row N = the flag under stop_rule, in both exit modes
 *   app        optional device float [N][F] (out): S;  iters: device int32 [F] (out), NULL allowed with BLDPC_EXIT_FIXED
 * Refused: codes built from an address table, block rows of weight < 2 and block rows of weight > 26 (BLDPC_EUNSUPPORTED; 26
 * is also the most bldpc_code_create_qc takes, which refuses a heavier matrix with the same code before a code object exists);
 * max_iter < 1, alpha outside (0, 1] or not finite, length outside [0, N], an unknown rule or mode, iters == NULL with
 * per-frame exit (BLDPC_EINVAL).  bldpc_decode_layered_host has no upper weight limit.  NaN inputs are undefined.
 * Asynchronous on `stream` in both exit modes; no allocation per call once the code object's scratch has grown (the layered
 * decoder keeps scratch of its own, apart from the flooding decoders').  bldpc_last_kernel names the tier that ran:
 * "k_lay_reg" / "k_lay" (all iterations on-chip: S in LDS, row states in registers / in LDS) or "k_lay_ws" (S and row states
 * in a device workspace: codes whose state exceeds the LDS, whose Z exceeds 1024 or whose N is not a multiple of 64). */
int bldpc_decode_layered(bldpc_code *code, const float *Channel_Out, int F, int max_iter, float alpha, int length, int exit_mode,
                         int stop_rule, int *D, float *app, int *iters, void *stream);

/* The same decoder on the host, all pointers host, no device needed: plain C++ that follows the steps above literally (one
 * R per edge), frames over at most 16 threads.  It is the statement of the semantics inside the product, as
 * bldpc_generator_host is for the encoder, and what the device kernels are tested against bit for bit.  NOT a fast path. */
int bldpc_decode_layered_host(int J, int L, int Z, const int *H, const float *Channel_Out, int F, int max_iter, float alpha,
                              int length, int exit_mode, int stop_rule, int *D, float *app, int *iters);

/* -- row-layered sum-product (belief propagation; not in the reference, whose check node is min-sum) ---------------- */

/* The schedule of bldpc_decode_layered with the exact check-node rule in place of the two minima, for codes made by
 * bldpc_code_create_qc.  Semantics, IEEE fp32, no fused multiply-add, no denormal flushing.
 *
 * Sum-product needs true LLRs.  The min-sum decoders are scale-invariant and take the raw channel value, so this entry point takes
 * a factor llr_scale: 2 / sigma^2 for the BPSK channels here, 1.0 after bldpc_qam_demap, which is already given 1 / (2 sigma^2).
 *
 *   Correction table.  T[k] is the fp32 nearest to log1p(exp(-(k + 0.5) / 16)), k = 0 .. 127: 128 literals in a header of its own
 *   (csrc/bldpc_bp_table.hpp), exported by bldpc_bp_table.  It is not computed at run time, so every machine carries the same bits.
 *     corr(x) for x >= 0:  x < 8.0f ? T[(int)(x * 16.0f)] : +0.0f        (the product is exact and the index is at most 127)
 *
 *   Box-plus.  bp(a, b):
 *     aa = |a|;  ab = |b|;  m = min(aa, ab);  p = aa + ab;  d = |aa - ab|
 *     r = (m + corr(p)) - corr(d), in exactly that order;  r = (r < 0) ? +0.0f : r
 *     the result has the bits of r, with the sign bit set to signbit(a) xor signbit(b); a -0.0f input counts as negative.
 *   The sum and difference are taken on the magnitudes, not on a +- b (with a +- b the correction has the wrong sign when the signs
 *   differ).
 *
 *   Decoder.  State per frame: S[v] = llr_scale * Channel_Out[v] (one fp32 product per value), R = +0.0f per edge.
 *   One iteration visits the block rows j = 0 .. J-1 in order; within a block row every t in 0 .. Z-1 is independent of the others;
 *   the edges i = 0 .. w-1 run in ascending block column, with v_i as in bldpc_decode_layered.  Per row:
 *     1. Q_i = S[v_i] - R_i
 *     2. F_0 = Q_0;  F_i = bp(F_{i-1}, Q_i) for i = 1 .. w-2
 *     3. B_{w-1} = Q_{w-1};  B_i = bp(Q_i, B_{i+1}) for i = w-2 .. 1
 *     4. R_0' = B_1;  R_{w-1}' = F_{w-2};  otherwise R_i' = bp(F_{i-1}, B_{i+1})
 *     5. S[v_i] = Q_i + R_i';  R_i' replaces R_i
 *   For w = 2 this gives R_0' = Q_1 and R_1' = Q_0 with no box-plus at all.
 *
 * Hard bits, flag, length, stop_rule (BLDPC_STOP_PREFIX or BLDPC_STOP_SYNDROME), exit_mode (BLDPC_EXIT_FIXED or
 * BLDPC_EXIT_PER_FRAME; BLDPC_EXIT_BATCH_GLOBAL refused), D, app (= S), iters and asynchrony are exactly those of
 * bldpc_decode_layered.
 * Refused with BLDPC_EINVAL: llr_scale not finite or <= 0, max_iter < 1, length outside [0, N], an unknown rule or mode,
 * iters == NULL with per-frame exit.  Refused with BLDPC_EUNSUPPORTED, with a message in bldpc_last_error: codes built from an
 * address table, block rows of weight < 2.  Inputs with |llr_scale * y| > 2^100, infinities and NaN are undefined.
 * No allocation per call once the code object's scratch has grown (scratch and workspace of its own, apart from the other
 * decoders').  bldpc_last_kernel names the tier that ran: "k_lbp" (all iterations on-chip: S and R of one or more frames in LDS,
 * 4 N + 4 E bytes per frame, E = edges; codes whose N is a multiple of 64, Z <= 1024 and of which one frame fits) or "k_lbp_ws"
 * (one workgroup per frame, S in place, R in a device workspace kept in the code object: every other code). */
int bldpc_decode_layered_bp(bldpc_code *code, const float *Channel_Out, int F, int max_iter, float llr_scale, int length,
                            int exit_mode, int stop_rule, int *D, float *app, int *iters, void *stream);

/* The same decoder on the host, all pointers host, no device needed: plain C++ that follows the steps above literally (one R per
 * edge), frames over at most 16 threads, no weight limit.  It is the statement of the semantics inside the product and what the
 * device kernels are tested against bit for bit.  NOT a fast path. */
int bldpc_decode_layered_bp_host(int J, int L, int Z, const int *H, const float *Channel_Out, int F, int max_iter, float llr_scale,
                                 int length, int exit_mode, int stop_rule, int *D, float *app, int *iters);

/* The correction table T[0 .. 127] of the two calls above (host pointer). */
int bldpc_bp_table(float T[128]);

/* -- quantised row-layered min-sum (finite word lengths; not in the reference) --------------------------------------- */

/* The word lengths of bldpc_decode_layered_quant.  llr_scale is an absolute gain on the channel value: min-sum is
 * scale-invariant, so it only sets the resolution of the quantiser (a value of y = 1.0 becomes the integer llr_scale). */
typedef struct bldpc_quant {
    float llr_scale;   /* finite, > 0: quantiser gain on the channel value */
    int bits_ch;       /* 2 .. bits_app   channel word:        C  = 2^(bits_ch-1)  - 1 */
    int bits_app;      /* bits_msg .. 15  a-posteriori word:   A  = 2^(bits_app-1) - 1 */
    int bits_msg;      /* 2 .. 8          check message word:  Mx = 2^(bits_msg-1) - 1 */
    int norm8;         /* 1 .. 8          normalisation in eighths (8 = none) */
    int offset;        /* 0 .. Mx         offset subtracted after normalisation */
} bldpc_quant;

/* The layered min-sum decoder a hardware designer sizes: finite word lengths, normalised and / or offset correction in integer
 * arithmetic, saturation at every store.  The schedule, the edge order, v_i, the flag rules, length, exit_mode
 * (BLDPC_EXIT_FIXED or BLDPC_EXIT_PER_FRAME; BLDPC_EXIT_BATCH_GLOBAL refused), stop_rule, D, iters and asynchrony are exactly
 * those of bldpc_decode_layered.  What differs, all in two's-complement integers:
 *
 *   Quantiser.  x = llr_scale * Channel_Out[v] (one fp32 product);
 *     S[v] = x >= (float)C ? C : x <= -(float)C ? -C : (int)rintf(x)      (ties to even: 0.5 -> 0, 1.5 -> 2, -0.5 -> 0, -2.5 -> -2)
 *   NaN is undefined.  R = 0 per edge.
 *   Per row:
 *     1. Q_i = S[v_i] - R_i                        (no clamp: |Q| <= A + Mx < 2^15 by the parameter ranges)
 *     2. sg_i = (Q_i < 0), zero is positive;  a_i = min(|Q_i|, Mx);  P = XOR of the sg_i;  m1 <= m2 the two smallest a_i with
 *        multiplicity;  first = lowest i with a_i == m1
 *     3. g(m) = max(0, ((m * norm8 + 4) >> 3) - offset);  mag_i = (i == first) ? g(m2) : g(m1)
 *        R_i' = (P xor sg_i) ? -mag_i : +mag_i
 *     4. S[v_i] = min(A, max(-A, Q_i + R_i'));  R_i' replaces R_i
 *   Hard bit d[v] = (S[v] < 0): S = 0 decodes to bit 0.
 *
 * The normalisation rounds: the smallest of the ~20 magnitudes of a rate-5/6 row is often 1, and (1 * 6) >> 3 would be 0.
 *   app  optional device int32 [N][F] (out): S
 * Refused with BLDPC_EINVAL and a message in bldpc_last_error: q == NULL, a parameter outside the ranges above, and the argument
 * errors of bldpc_decode_layered.  Refused with BLDPC_EUNSUPPORTED: codes built from an address table, block rows of weight < 2.
 * No allocation per call once the code object's scratch has grown (scratch and workspace of its own, apart from the other
 * decoders').  Two frames share every 32-bit word and every packed 16-bit instruction; with odd F the last frame runs alone.
 * bldpc_last_kernel names the tier that ran: "k_lq" (all iterations on-chip: per frame pair 4 N bytes of S and 16 bytes per
 * check row in LDS; codes with Z <= 1024 of which one pair, 4 N + 16 J Z + 16 bytes, fits the 159 KiB a workgroup may ask for) or
 * "k_lq_ws" (one workgroup per frame pair, S in place, row states in a device workspace kept in the code object: every other
 * code). */
int bldpc_decode_layered_quant(bldpc_code *code, const float *Channel_Out, int F, int max_iter, const bldpc_quant *q,
                               int length, int exit_mode, int stop_rule, int *D, int *app, int *iters, void *stream);

/* The same decoder on the host, all pointers host, no device needed: plain C++ that follows the steps above literally (one R per
 * edge), frames over at most 16 threads, no upper weight limit.  It is the statement of the semantics inside the product and what
 * the device kernels are tested against bit for bit.  NOT a fast path. */
int bldpc_decode_layered_quant_host(int J, int L, int Z, const int *H, const float *Channel_Out, int F, int max_iter,
                                    const bldpc_quant *q, int length, int exit_mode, int stop_rule, int *D, int *app, int *iters);

/* -- normalised min-sum on the flooding decoders (not in the reference, whose flooding min-sum is un-normalised) ----- */

/* The flooding iteration exactly as bldpc_decode runs it, with one change in the check-node update.  Semantics, IEEE fp32
 * without fused multiply-add and without flushing denormals:
 *
 *   state per frame: one message word per edge, R = +0.0f (Memory_RQ = 0, LDPC_Decoder.cu:82).
 *   one iteration:
 *     1. variable nodes (LDPC_Decoder.cu:188-210): for every variable v with edges e_0 .. e_{w-1} in ascending block row,
 *        S[v] = (((0 + R_0) + R_1) + ...) + Channel_Out[v];  Q_i = S[v] - R_i replaces R_i on every edge
 *     2. hard bits d[v] = S[v] < 0;  the frame's flag = no d[v] is 1 among the first `length` variables (0 means K = N - M)
 *     3. the decoder stops here after max_iter iterations, and a frame under per-frame exit at its first set flag: the
 *        check-node pass after the last variable-node pass is not executed
 *     4. check nodes (:279-314): for every check with edges i = 0 .. w-1 in ascending block column,
 *        sg_i = Q_i < 0 ? -1 : +1;  P = product of all sg_i;  a_i = |Q_i|;  m1 <= m2 the two smallest a_i with multiplicity;
 *        first = lowest i with a_i == m1
 *        mag_i = alpha * (i == first ? m2 : m1)          (one fp32 multiplication: the only change)
 *        R_i = (float)(P * sg_i) * mag_i  replaces Q_i   (a multiplication by +-1: the bits of +-mag_i)
 *
 *   With alpha == 1.0f the results are those of bldpc_decode (BLDPC_EXIT_FIXED) and bldpc_decode_per_frame bit for bit:
 *   x * 1.0f is exact, signed zeros and denormals included.  An underflowing product makes R_i = +-0 where the minimum is not 0;
 *   S is still never -0.0f (it is accumulated from +0.0f) and Q = S - R never is either.
 *
 *   exit_mode  BLDPC_EXIT_FIXED or BLDPC_EXIT_PER_FRAME (iters[f] and column f of D and app as bldpc_decode_per_frame returns them).
 *              BLDPC_EXIT_BATCH_GLOBAL is refused (BLDPC_EINVAL), as the layered decoder refuses it.
 *   alpha      normalisation factor in (0, 1]; outside it or not finite: BLDPC_EINVAL
 *   iters      device int32 [F] (out) with per-frame exit, where NULL is refused (BLDPC_EINVAL); not written with BLDPC_EXIT_FIXED
 * All other arguments, layouts, scratch and asynchrony are those of bldpc_decode and bldpc_decode_per_frame; there is no flag
 * history.  The call always runs the normalised instantiations of the kernels, at alpha == 1.0f too, and bldpc_last_kernel
 * reports the name the plain path reports for that tier with "_norm" appended.  Codes built from an address table are accepted and
 * run the table kernels.  One corner has no fused normalised kernel: the per-frame exit of a row-local plan WITHOUT a nested plain
 * plan (a pinned entry, BLDPC_LOCAL_PER_FRAME); BLDPC_KERNEL_AUTO runs the table kernels there ("table_vec4_norm"), an explicit
 * BLDPC_KERNEL_QC_LDS is refused with BLDPC_EUNSUPPORTED. */
int bldpc_decode_normalised(bldpc_code *code, const float *Channel_Out, int F, int max_iter, float alpha, int length,
                            int exit_mode, int kernel, int *D, float *app, int *iters, void *stream);

/* The same decoder on the host for QC codes, all pointers host, no device needed: plain C++ that follows the steps above
 * literally (one R per edge), frames over at most 16 threads.  It is the statement of the semantics inside the product, as
 * bldpc_decode_layered_host is for the layered decoder, and what the normalised kernels are tested against bit for bit.  Block
 * rows of weight < 2 are refused (BLDPC_EUNSUPPORTED).  iters may be NULL with BLDPC_EXIT_FIXED.  NOT a fast path. */
int bldpc_decode_normalised_host(int J, int L, int Z, const int *H, const float *Channel_Out, int F, int max_iter, float alpha,
                                 int length, int exit_mode, int *D, float *app, int *iters);

/* -- binary codes over QAM: bit mapper and max-log soft demapper (not in the reference, whose binary channel is BPSK) -- */

/* Bit-interleaved coded modulation without the interleaver: m consecutive codeword bits label one of q = 2^m constellation
 * points, 1 <= m <= 8.  Semantics:
 *
 *   constellation  float [q][2] (Real, Imag), as nbldpc_read_constellation returns it
 *   Ns = ceil(N / m) symbols per frame.  Bit b (0 <= b < m) of symbol s is codeword bit n = s*m + b and is bit b of the point
 *   index: idx = sum_b bit[s*m + b] << b (only bit 0 of a CodeWord entry is read, as in bldpc_encode).  This is the order in which
 *   the GF(q) channels read a symbol's bits (nbldpc_awgn_channel_device[_qam]_frames); the shipped GRAY_*QAM.txt files are Gray in
 *   these index bits.  Positions n >= N of the last symbol are pad bits: they are sent as 0, the demapper writes nothing for them
 *   and makes no use of knowing them.  These two calls have NO interleaver: neighbouring codeword bits share a symbol.  The _il
 *   calls below take the index rule as an argument.
 *
 *   map:    sym[f][s] = idx, int32 [F][Ns] -- what nbldpc_awgn_channel_device_qam_frames takes as CodeWord_sym with its N := Ns.
 *           CodeWord == NULL is the all-zero word: every index is 0.
 *   demap:  max-log, IEEE fp32 without fused multiply-add.  For the received point (x, y) = rx[f][s] and every point p:
 *             dx = x - cx_p;  dy = y - cy_p;  d_p = dx*dx + dy*dy         (two multiplications, one addition)
 *           and for every bit b with s*m + b < N:
 *             m0 = min{d_p : bit b of p is 0};  m1 = min{d_p : bit b of p is 1}
 *             Channel_Out[(s*m + b)*F + f] = (m1 - m0) * scale             (one subtraction, one multiplication)
 *           Positive means bit 0, as with the BPSK channel's y = 1 - 2c.  A minimum is a selection, so the order in which the
 *           points are visited does not change the bits.  NaN inputs are undefined.
 *   scale   caller-supplied fp32: 1 / (2 sigma^2) gives true (max-log) LLRs; 1.0f serves the min-sum decoders of this library
 *           as well, which are scale-invariant (every message is a sum or a minimum of inputs, times alpha).
 *
 * The three calls of one batch over the QAM channel, on the reference's noise stream:
 *     bldpc_qam_map(CodeWord, N, F, m, sym, stream);
 *     nbldpc_awgn_channel_device_qam_frames(seed, sigma, sym, Ns, constellation, q, F, rx, stream);   // include/nbldpc.h: 4 draws per
 *                                                                             // symbol, advances seed by 4*Ns*F draws
 *     bldpc_qam_demap(rx, constellation, q, 1.0f / (2 * sigma * sigma), N, F, Channel_Out, stream);
 * with sigma = nbldpc_sigma(SNR, snrtype, q, rate) (its quirks included), so that a binary and a GF(q) sweep at one SNR value run
 * at the same sigma.
 *
 *   CodeWord     device int32 [N][F] or NULL     sym          device int32 [F][Ns]
 *   rx           device float [F][Ns][2]         constellation device float [q][2]      Channel_Out  device float [N][F]
 * Both calls are asynchronous on `stream` and allocate nothing.  BLDPC_EINVAL: a null pointer (but CodeWord), N or F <= 0, m
 * outside 1..8, q not a power of two in 2..256, scale not finite.
 * Out of scope: the exact log-sum-exp demapper (its expf / logf differ between device and host libm in the last ulp, which would end
 * bit-exact testing for a small gain under Gray labelling), interleavers other than the row-column one below, iterative demapping. */
int bldpc_qam_map(const int *CodeWord, int N, int F, int m, int *sym, void *stream);
int bldpc_qam_demap(const float *rx, const float *constellation, int q, float scale, int N, int F, float *Channel_Out, void *stream);

/* The bit interleaver, as an index rule inside the modem: which of the N bits is bit b of symbol s (Ns = ceil(N / m)).
 *   BLDPC_IL_NONE    e = s*m + b    the rule of bldpc_qam_map / bldpc_qam_demap; the _il calls then give their bits
 *   BLDPC_IL_ROWCOL  e = b*Ns + s   the row-column interleaver: the bits are written row by row into m rows of Ns and read column by
 *                                   column, so that the m bits of a symbol lie Ns positions apart in the word
 * In both rules e >= N is a pad bit: sent as 0, no output.  With N % m != 0 the pads of ROWCOL are the upper bits of the last
 * symbols, one per symbol, not the tail of the last symbol; this keeps every N legal.  Index bit b keeps its meaning (bit b of the
 * point index), and everything else is as said above, argument checks included; interleave outside {0, 1} is BLDPC_EINVAL. */
#define BLDPC_IL_NONE 0
#define BLDPC_IL_ROWCOL 1
int bldpc_qam_map_il(const int *CodeWord, int N, int F, int m, int interleave, int *sym, void *stream);
int bldpc_qam_demap_il(const float *rx, const float *constellation, int q, float scale, int N, int F, int interleave, float *Channel_Out,
                       void *stream);
int bldpc_qam_map_il_host(const int *CodeWord, int N, int F, int m, int interleave, int *sym);
int bldpc_qam_demap_il_host(const float *rx, const float *constellation, int q, float scale, int N, int F, int interleave, float *Channel_Out);

/* The same on host pointers, no device needed (and so no stream: they return when done): plain C++ that follows the steps above
 * literally.  They are the statement of the semantics inside the product, as bldpc_decode_layered_host is for the layered decoder,
 * and what the kernels are tested against bit for bit.  Same argument checks. */
int bldpc_qam_map_host(const int *CodeWord, int N, int F, int m, int *sym);
int bldpc_qam_demap_host(const float *rx, const float *constellation, int q, float scale, int N, int F, float *Channel_Out);

/* -- block fading with receiver CSI (not in the reference, whose channels are memoryless AWGN) ----------------------------- */

/* Model: flat Rayleigh block fading, perfect receiver CSI, coherent detection.  A channel use is a bit over BPSK and a constellation
 * point over QAM.  Use s of frame f has a real gain a[f][s] >= 0 that the receiver knows; it receives r = a * x + n with n exactly the
 * noise the AWGN channels draw.  E[a^2] = 1, so sigma under Es/N0 and Eb/N0 stays what bldpc_sigma / nbldpc_sigma give.
 *
 * The gain array is always float [F][S], frame outer, one entry per channel use.  The block structure lives in the generator below
 * only: every consumer reads a plain per-use gain, so a caller may supply any other fading process.  A consumer requires finite
 * gains >= 0 and nothing else; other values are undefined, as NaN inputs are.
 *
 * (a) Gains.  nb = ceil(S / Lc) blocks per frame.  Block j of frame f takes draw number f * nb + j of the RandomModule stream at
 * `seed`, one draw u, and a = sqrtf(-logf(1.0f - u)) is written to gain[f*S + s] for every s with s / Lc == j.  seed advances by
 * nb * F draws.  Lc >= 1; Lc = 1 is fast fading; Lc >= S (Lc > S is legal) is one block, quasi-static fading.  1 - u >= 2^-24, so
 * 0 <= a <= 4.08.  The fading stream has a seed triple of its own, separate from the noise seed: a frame's gains and a frame's noise
 * then depend on the frame's global index only, not on the batch size or on the number of ranks.  The device call jumps
 * every thread to its first draw as bldpc_awgn_channel_device does (same draws; device libm, so a gain is the host's or an ulp away).
 *   gain  device (host: host) float [F][S]      BLDPC_EINVAL: a null pointer, Lc < 1, S or F <= 0, a seed outside its modulus */
int bldpc_fading_gains_device(int seed[3], int Lc, int S, int F, float *gain, void *stream);
int bldpc_fading_gains_host(int seed[3], int Lc, int S, int F, float *gain);

/* (b) BPSK channel.  The draws, their indexing (2 (f*N + n)) and the seed advance are those of bldpc_awgn_channel_device.  With
 * a = gain[f*N + n]:
 *     r = (float)((double)sigma * sin(two_pi * (double)u2) * (double)amp + (double)a * (1.0 - (double)(2*c)))
 *     Channel_Out[n*F + f] = a * r            one fp32 multiplication: the matched-filter value
 * so that 2 / sigma^2 stays the sum-product decoder's llr_scale.  gain [F][N]; CodeWord == NULL is the all-zero word.  With
 * a == 1.0f this is bldpc_awgn_channel_device's value bit for bit.  BLDPC_EINVAL: a null seed, gain or Channel_Out, N or F <= 0, a
 * seed outside its modulus (the host statement included). */
int bldpc_awgn_fading_channel_device(int seed[3], float sigma, const float *gain, float *Channel_Out, const int *CodeWord, int N, int F,
                                     void *stream);
int bldpc_awgn_fading_channel_host(int seed[3], float sigma, const float *gain, float *Channel_Out, const int *CodeWord, int N, int F);

/* (d) The max-log demapper with CSI: everything bldpc_qam_demap_il says, with the distances taken to the faded points,
 *     dx = x - a*cx_p;  dy = y - a*cy_p;  d_p = dx*dx + dy*dy         a = gain[f*Ns + s], aligned with rx [F][Ns][2]
 * two more fp32 multiplications per point, no fused multiply-add, no division, no special case.  a == 0 makes all distances equal and
 * every output +0.0f: an erasure.  a == 1.0f gives bldpc_qam_demap_il's bits.  The equalised form (divide the point by a, weight the
 * result by a^2) is deliberately not the specification: it overflows for small gains and needs a special case at 0.
 * The QAM channel that applies the gains is nbldpc_fading_channel_device_qam_frames (include/nbldpc.h).  Same argument checks as
 * bldpc_qam_demap_il, and gain != NULL.
 *
 * Rate matching and HARQ over a fading channel are compositions, through an [E][F] array:
 *     BPSK   bldpc_rm_select -> bldpc_awgn_fading_channel_device at N := E -> bldpc_rm_recover / bldpc_rm_combine
 *            (sample (f, e) uses the draws 2 (f E + e), as the fused rate-matched channel does)
 *     QAM    bldpc_rm_qam_map -> nbldpc_fading_channel_device_qam_frames -> bldpc_qam_demap_fading at N := E with the interleave rule
 *            -> bldpc_rm_recover / bldpc_rm_combine       (the composition bldpc_rm_qam_recover is defined by)
 * Fused fading forms of bldpc_rm_awgn_* and bldpc_rm_qam_* are out of scope, as are complex gains, phase errors, imperfect CSI and
 * correlated (Doppler) processes -- the last can be had by passing a gain array of one's own. */
int bldpc_qam_demap_fading(const float *rx, const float *gain, const float *constellation, int q, float scale, int N, int F, int interleave,
                           float *Channel_Out, void *stream);
int bldpc_qam_demap_fading_host(const float *rx, const float *gain, const float *constellation, int q, float scale, int N, int F, int interleave,
                                float *Channel_Out);

/* -- rate matching: shortened and punctured codes (not in the reference, which transmits every bit of the mother code) -- */

/* A profile over a mother code of N bits names two disjoint sets of codeword positions.  Semantics:
 *
 *   shortened   the bit is 0 by agreement and is not sent; the receiver knows it: its channel value is short_llr, a large
 *               positive confidence (positive means bit 0, as with y = 1 - 2c).
 *   punctured   the bit is whatever the encoder made it and is not sent; the receiver knows nothing: its channel value is +0.0f.
 *   transmitted every other position, E = N - n_short - n_punct of them, in ascending codeword position:
 *               tx_pos[0] < ... < tx_pos[E-1].  The rate of the derived code is (K - n_short) / E.
 *
 *   select:   tx[e][f] = CodeWord[tx_pos[e]][f]                                  a gather; the shortened rows are not looked at
 *   recover:  Channel_Out[n][f] = rx[e][f]     (the same 32 bits)                 n = tx_pos[e]
 *                               = +0.0f        (0x00000000)                       n punctured
 *                               = short_llr                                       n shortened
 *             the de-rate-matcher for values from any source, bldpc_qam_demap included (run the modem with N := E)
 *   channel:  recover(bldpc_awgn_channel(select(CodeWord)) with N := E) as ONE pass: noise is drawn for the transmitted bits only, on
 *             the reference's stream -- sample (f, e) uses draws 2(f*E + e) and 2(f*E + e) + 1 of RandomModule, in the arithmetic of
 *             bldpc_awgn_channel_host / _device, and seed[3] advances by 2*E*F draws.  The device version writes [N][F] from one
 *             kernel, with no [E][F] intermediate; its transmitted rows carry the bits bldpc_awgn_channel_device gives for N := E
 *             on the selected codeword, the host version those of bldpc_awgn_channel_host.
 *
 * Every decoder of this library takes such an input as it stands: nothing in a min-sum iteration treats 0 or a large value apart.
 * short_llr must be finite and > 0 (BLDPC_EINVAL).  +inf is refused on purpose: a check all of whose other neighbours are shortened
 * sends inf, and the next S - R is inf - inf.  The min-sum decoders are scale-invariant, so any value far above the channel's serves.
 *
 *   CodeWord     device int32 [N][F] (the channel: or NULL = the all-zero word)      tx   device int32 [E][F]
 *   rx           device float [E][F]                                                Channel_Out  device float [N][F]
 * All arrays frame-fastest.  The device calls are asynchronous on `stream` and allocate nothing per call (the profile's device
 * tables are uploaded by the first of them: use a profile from one host thread at a time, like a code object).
 * Out of scope: hard-decision (BSC) input, the position lists of any standard.  (Rate matching and HARQ over QAM: "rate matching
 * over QAM" below.  The GF(q) half reads the same profile over code symbols: include/nbldpc.h, "rate matching".) */
typedef struct bldpc_rm bldpc_rm; /* opaque: the kind of every position, its rank among the transmitted ones, tx_pos; host + device */

/* Positions are codeword positions in [0, N), in any order.  BLDPC_EINVAL: a position out of range, a position repeated or present
 * in both lists, E < 1, a null list with a non-zero count, a negative count, N < 1 or N > 2 097 120 (the launch grid of the kernels).
 * Both counts zero is the identity profile.  Host only: no device is touched until the first device call on the profile. */
int bldpc_rm_create(int N, const int *short_pos, int n_short, const int *punct_pos, int n_punct, bldpc_rm **rm);
int bldpc_rm_destroy(bldpc_rm *rm);
int bldpc_rm_dims(const bldpc_rm *rm, int dims[4]);   /* N, E, n_short, n_punct */
int bldpc_rm_tx_pos(const bldpc_rm *rm, int *tx_pos); /* host int [E] */

int bldpc_rm_select(const bldpc_rm *rm, const int *CodeWord, int F, int *tx, void *stream);
int bldpc_rm_recover(const bldpc_rm *rm, const float *rx, int F, float short_llr, float *Channel_Out, void *stream);
/* seed[3]: host, every state in [0, m) as for bldpc_awgn_channel_device (BLDPC_EINVAL otherwise), advanced in place. */
int bldpc_rm_awgn_channel_device(const bldpc_rm *rm, int seed[3], float sigma, const int *CodeWord, int F, float short_llr,
                                 float *Channel_Out, void *stream);

/* The same on host pointers, no device needed (and so no stream: they return when done): plain C++ that follows the steps above
 * literally -- the channel IS select, bldpc_awgn_channel_host with N := E, recover.  They are the statement of the semantics inside
 * the product and what the kernels are tested against bit for bit.  Same argument checks (any int triple is a seed here, as for
 * bldpc_awgn_channel_host). */
int bldpc_rm_select_host(const bldpc_rm *rm, const int *CodeWord, int F, int *tx);
int bldpc_rm_recover_host(const bldpc_rm *rm, const float *rx, int F, float short_llr, float *Channel_Out);
int bldpc_rm_awgn_channel_host(const bldpc_rm *rm, int seed[3], float sigma, const int *CodeWord, int F, float short_llr,
                               float *Channel_Out);

/* bldpc_encode_random with shortened bits: the message rule of bldpc_encode_random, then every message bit k whose info_pos[k] is a
 * shortened position of `rm` is forced to 0, then the encoding; msg (when not NULL) receives the messages after the forcing.  Frame g
 * is still the same codeword at any world size.  BLDPC_EINVAL: rm's N differs from the code's, or a shortened position is not an
 * information position of the code's generator (a parity bit is determined by the message and cannot be agreed to be 0).
 * Punctured positions play no part.  Other arguments, limits and asynchrony as bldpc_encode_random. */
int bldpc_rm_encode_random(bldpc_code *code, const bldpc_rm *rm, unsigned long long seed, long long first_frame, int F, int *msg,
                           int *CodeWord, void *stream);

/* -- HARQ: circular-buffer rate matching, soft combining, frame compaction (not in the reference) -- */

/* A circular profile reads the BUFFER of a profile -- the Ncb = N - n_short - n_punct positions that are neither shortened nor
 * punctured, ascending, buf[0..Ncb), what bldpc_rm_create calls the transmitted positions -- from a redundancy-version start k0 for
 * E positions, around the end and as often as E asks:
 *
 *   tx_pos[e] = buf[(k0 + e) mod Ncb],  0 <= e < E       no longer ascending; E > Ncb repeats positions, E < Ncb leaves the positions
 *                                                       not reached without a sample in this transmission; punctured positions are
 *                                                       never sent by any transmission
 *   Position n of rank b in the buffer (buf[b] = n) has the contributions e_0 = (b - k0) mod Ncb, e_0 + Ncb, e_0 + 2 Ncb, ... < E.
 *
 *   select:   tx[e][f] = CodeWord[tx_pos[e]][f]
 *   recover:  Channel_Out[n][f] = the 32 bits of rx[e_0][f], then + rx[e_1][f], then + rx[e_2][f], ...: fp32 additions in ascending
 *             e, not contracted, not reordered.  With one contribution this is the copy of a linear profile (-0.0f and NaN payloads
 *             survive); the sum does not start from zero, so -0.0f sent twice gives -0.0f.
 *                               = 0x00000000   no contribution: n punctured or not reached
 *                               = short_llr    n shortened
 *   combine:  Channel_Acc[n][f] (read and written), for every frame with done[f] == 0 (done == NULL: every frame):
 *                               = ((acc + rx[e_0][f]) + rx[e_1][f]) + ...    starting from the stored value
 *                               unchanged      no contribution
 *                               = short_llr    n shortened
 *             A frame with done[f] != 0 is not touched at all: its column keeps its bits.  done may be row N of a decoder's D after
 *             bldpc_syndrome (or a decoder with BLDPC_STOP_SYNDROME) wrote the flag there.
 *             The first transmission of a codeword is recover, every later one is combine.  The same profile twice is Chase
 *             combining, profiles of different k0 are incremental redundancy.  rx may come from any source: with bldpc_qam_demap
 *             run at N := E on the selected bits, combine is HARQ over QAM ("rate matching over QAM" below does it in one pass).
 *   channel:  bldpc_rm_awgn_channel_device / _host on a circular profile: sample (f, e) uses draws 2(f*E + e) and 2(f*E + e) + 1 in the
 *             arithmetic of bldpc_awgn_channel_device / _host, seed[3] advances by 2*E*F draws, the output is recover of those samples.
 *   channel + combine:  the same samples combined into Channel_Acc under done, ONE kernel, no [E][F] intermediate.  The draws of a done
 *             frame are skipped, not handed to another frame, and seed[3] advances by 2*E*F whatever done holds: a frame's noise
 *             depends neither on its batch mates nor on the world size.
 *
 * bldpc_rm_create_circular refuses (BLDPC_EINVAL) everything bldpc_rm_create refuses, k0 outside [0, Ncb), E < 1, E > 8 * Ncb (the
 * fused kernel keeps one generator state per lap of the buffer in registers, eight at most) and E > 2 097 120 (the launch grid of a
 * kernel that walks E rows).  bldpc_rm_dims reports this E, bldpc_rm_tx_pos the E entries in transmission order, and the rate
 * (K - n_short) / E is that of this one transmission.  No device table is added: the profile's one table still holds the rank b.
 * A profile from bldpc_rm_create is the circular profile k0 = 0, E = Ncb.  In the entry points it had before (select, recover, channel)
 * it runs the kernels it ran before; bldpc_rm_combine and bldpc_rm_awgn_combine_device take both kinds.
 *
 *   rx           device float [E][F]            done         device int32 [F] or NULL
 *   Channel_Acc  device float [N][F]            CodeWord     device int32 [N][F] or NULL = the all-zero word
 * Asynchronous on `stream`, nothing allocated per call; checks of short_llr, seed and F as in "rate matching". */
int bldpc_rm_create_circular(int N, const int *short_pos, int n_short, const int *punct_pos, int n_punct, int k0, int E, bldpc_rm **rm);
int bldpc_rm_circ(const bldpc_rm *rm, int info[4]); /* Ncb, k0, E, laps = ceil(E / Ncb); a linear profile: Ncb, 0, Ncb, 1 */
int bldpc_rm_combine(const bldpc_rm *rm, const float *rx, int F, float short_llr, const int *done, float *Channel_Acc, void *stream);
int bldpc_rm_awgn_combine_device(const bldpc_rm *rm, int seed[3], float sigma, const int *CodeWord, int F, float short_llr, const int *done,
                                 float *Channel_Acc, void *stream);
/* Host statements (all pointers host, no device needed): plain C++ that follows the words above literally; channel + combine IS
 * select, bldpc_awgn_channel_host with N := E, combine.  bldpc_rm_select_host, bldpc_rm_recover_host and bldpc_rm_awgn_channel_host
 * take a circular profile as their device twins do. */
int bldpc_rm_combine_host(const bldpc_rm *rm, const float *rx, int F, float short_llr, const int *done, float *Channel_Acc);
int bldpc_rm_awgn_combine_host(const bldpc_rm *rm, int seed[3], float sigma, const int *CodeWord, int F, float short_llr, const int *done,
                               float *Channel_Acc);

/* -- rate matching over QAM: select + interleave + map, and demap + de-interleave + recover / combine, one pass each -- */

/* A rate-matched transmission over QAM sends the profile's E bits through the modem at N := E.  Each call below is, bit for bit, a
 * composition of calls above, without the [E][F] array between them:
 *
 *   bldpc_rm_qam_map:      bldpc_rm_select into tx[E][F], then bldpc_qam_map_il(tx, E, F, m, interleave, sym).  Bit b of symbol s is
 *                          read at CodeWord[tx_pos[e]][f], e by the index rule.  CodeWord == NULL is the all-zero word.
 *   bldpc_rm_qam_recover:  bldpc_qam_demap_il(rx, ..., N := E, ..., tmp), then bldpc_rm_recover(rm, tmp, F, short_llr, Channel_Out).
 *   bldpc_rm_qam_combine:  the same demap, then bldpc_rm_combine(rm, tmp, F, short_llr, done, Channel_Acc).
 *
 * with everything "rate matching" and "HARQ" say of recover and combine: a position's contributions are added in fp32 in ascending
 * e, not contracted; recover starts from the first sample's bits; a position without a contribution is 0x00000000 (recover) or is
 * not touched (combine); shortened positions are short_llr; a frame with done[f] != 0 keeps every bit of its column.  The three take
 * linear and circular profiles.  On the device a profile of several laps is one launch of the demapper per lap, in stream order
 * (launch l commits the bits l*Ncb <= e < (l+1)*Ncb, inside which no position comes twice; under BLDPC_IL_ROWCOL every launch walks
 * all symbols); one lap is one launch, after one small launch that fills the rows the demapper does not reach when there are any.
 * With scale = 1 / (2 sigma^2) the accumulated values are true max-log LLRs of the combined transmissions.
 *
 *   sym          device int32 [F][Ns], Ns = ceil(E / m)      rx   device float [F][Ns][2], as nbldpc_awgn_channel_device_qam_frames writes it
 *   Channel_Out, Channel_Acc  device float [N][F]             done device int32 [F] or NULL       constellation device float [q][2]
 * Asynchronous on `stream`, nothing allocated per call (the profile's tables are uploaded by its first device call).  BLDPC_EINVAL:
 * what the modem calls and bldpc_rm_recover / bldpc_rm_combine refuse, and interleave outside {0, 1}; a refused call launches nothing.
 * The _host twins ARE the compositions, on the host statements (bldpc_rm_select_host, bldpc_qam_map_il_host, bldpc_qam_demap_il_host,
 * bldpc_rm_recover_host, bldpc_rm_combine_host); they allocate the [E][F] array (BLDPC_ENOMEM). */
int bldpc_rm_qam_map(const bldpc_rm *rm, const int *CodeWord, int F, int m, int interleave, int *sym, void *stream);
int bldpc_rm_qam_recover(const bldpc_rm *rm, const float *rx, const float *constellation, int q, float scale, int interleave, int F,
                         float short_llr, float *Channel_Out, void *stream);
int bldpc_rm_qam_combine(const bldpc_rm *rm, const float *rx, const float *constellation, int q, float scale, int interleave, int F,
                         float short_llr, const int *done, float *Channel_Acc, void *stream);
int bldpc_rm_qam_map_host(const bldpc_rm *rm, const int *CodeWord, int F, int m, int interleave, int *sym);
int bldpc_rm_qam_recover_host(const bldpc_rm *rm, const float *rx, const float *constellation, int q, float scale, int interleave, int F,
                              float short_llr, float *Channel_Out);
int bldpc_rm_qam_combine_host(const bldpc_rm *rm, const float *rx, const float *constellation, int q, float scale, int interleave, int F,
                              float short_llr, const int *done, float *Channel_Acc);

/* Frame compaction: the columns idx[0] < idx[1] < ... < idx[Fa-1] of an array [rows][F] of 32-bit words of any meaning (a decoder's
 * float input, its int32 D with rows = N + 1, iters with rows = 1):
 *   gather:   dst[r][a] = src[r][idx[a]]      src [rows][F],  dst [rows][Fa]
 *   scatter:  dst[r][idx[a]] = src[r][a]      src [rows][Fa], dst [rows][F]; the other columns of dst are not touched
 * idx is device int32 [Fa], strictly ascending in [0, F): a precondition of the device calls (an index outside [0, F) moves nothing, a
 * repeated one makes scatter's result undefined), checked by the host twins (BLDPC_EINVAL).  The per-frame results of BLDPC_EXIT_FIXED
 * and BLDPC_EXIT_PER_FRAME do not depend on a frame's batch mates, so decoding the gathered unacknowledged frames and scattering D and
 * iters back gives the bits of decoding every frame again.  BLDPC_EINVAL: a null pointer, Fa < 1, Fa > F, rows < 1 or > 2 097 120.
 * The list comes from the caller (in Python: torch.nonzero on the flag row). */
int bldpc_frames_gather(const void *src, int rows, int F, const int *idx, int Fa, void *dst, void *stream);
int bldpc_frames_scatter(const void *src, int rows, int F, const int *idx, int Fa, void *dst, void *stream);
int bldpc_frames_gather_host(const void *src, int rows, int F, const int *idx, int Fa, void *dst);
int bldpc_frames_scatter_host(const void *src, int rows, int F, const int *idx, int Fa, void *dst);

/* sigma of the sweep point (main.cu:120-127): snrtype 0 = Eb/N0 (uses rate), 1 = Es/N0. */
float bldpc_sigma(float SNR, int snrtype, float rate);

/* Timing of the dominant kernel (k_qc / k_qc2, or the VN+CN launch sequence of the table kernels) with
 * HIP events on the stream the kernel runs on.  enable != 0 makes every following bldpc_decode record a
 * pair of events around that kernel; bldpc_last_kernel_ms waits for the last pair and returns the
 * elapsed milliseconds in *ms.  Used by bench.py for the roofline line; off by default. */
int bldpc_set_profiling(bldpc_code *code, int enable);
int bldpc_last_kernel_ms(bldpc_code *code, float *ms);
/* Mean over the decode calls made since the previous bldpc_kernel_ms_mean / bldpc_set_profiling (at most the last 64): every
 * profiled call records its own event pair, nothing synchronises until this function is called.  *launches = calls averaged. */
int bldpc_kernel_ms_mean(bldpc_code *code, float *mean_ms, int *launches);

/* Name of the kernel variant the last bldpc_decode / bldpc_decode_layered / bldpc_decode_layered_bp / bldpc_decode_layered_quant on
 * this code used (static string). */
const char *bldpc_last_kernel(const bldpc_code *code);

/* -- the table of fused (QC_LDS) kernel variants, read-only ---------------------------------------------------------- */

/* The fused kernels are instantiated ahead of time, one table entry ("variant") per geometry; a code object takes the first
 * entry that accepts its matrix (BLDPC_QC_VARIANT=<index> in the environment, read when the code is created, pins one).
 * These calls only report; they select nothing.  Host only: no device is touched.
 *   bldpc_qc_variant_count   entries in the table
 *   bldpc_qc_variant_info    info[16] of entry `index` (0 <= index < count, else BLDPC_EINVAL):
 *     [0] NF frames per lane  [1] J  [2] L  [3] Z   (J = L = 0: any; L = 0: any)
 *     [4] WC heaviest block row taken  [5] WV heaviest block column taken (31: no limit of the entry's own)
 *     [6] G thread groups  [7] MINW lightest block row taken (checked by the register-state entries only)
 *     [8] CPT block columns per thread group at most (compressed entries) or NG, the wrapped blocks per (row, tile) at most
 *         (register-state entries with halos); 0 elsewhere
 *     [9] regstate: 0, 1 = check states in registers, 2 = the same with halo columns
 *     [10] loc: 0, 1 = half-row kernel with local edges, 2 = row kernel with local edges
 *     [11] 1 when the entry has a persistent per-frame kernel  [12] U lanes per thread group (compressed entries, else 0)
 *     [13] threads per workgroup  [14] LDS bytes (0: computed per code)  [15] 0
 *     *tag (when not NULL): the entry's tag as it appears in bldpc_last_kernel ("row", "halfrow", "compressed", ...), static. */
int bldpc_qc_variant_count(void);
int bldpc_qc_variant_info(int index, int info[16], const char **tag);

/* What the fused-kernel plan of a code object is, info[8]:
 *   [0] variant index of the plan, -1: none (the table kernels serve the code)
 *   [1] variant index of the nested plan that serves the per-frame passes, -1: none (the plan itself serves them)
 *   [2] persist_grid: workgroups of the plan's persistent kernel (0: it has none)  [3] frames per workgroup
 *   [4] 1 when built under BLDPC_REGROUP  [5] 1 when built under BLDPC_NO_PERSIST
 *   [6] persist_grid of the nested plan (0: none)  [7] 0 */
int bldpc_code_qc_info(const bldpc_code *code, int info[8]);

/* The plan bldpc_code_create_qc would make for the block matrix H [J][L] (shifts, -1 = zero block), without a device: the table
 * entry and the tables its kernel reads, as digests.  pin: a variant index as in BLDPC_QC_VARIANT, -1 = none.  flags: bit 0
 * BLDPC_NO_LOCAL, bit 1 BLDPC_NO_HALO, bit 2 BLDPC_LOCAL_PER_FRAME (the other switches change no table).
 *   info[8]    [0] variant, -1: none  [1] variant of the nested per-frame plan, -1: none  [2] LDS bytes  [3] lc, the block column the
 *              register-state kernels keep in registers  [4] WVS, padded column list length of the compressed-state kernel
 *              [5] frames per workgroup  [6] [7] 0
 *   digest[8]  [0..6] 64-bit FNV-1a (offset basis 1469598103934665603, prime 1099511628211) of the bytes handed to the device as
 *              cn, rowptr, vn, wv, cn_meta, vn_meta, lane; 0 for a table that is not uploaded
 *              [7] FNV-1a of the nested plan's seven digests (56 bytes, as stored), 0: no nested plan */
int bldpc_qc_plan_host(int J, int L, int Z, const int *H, int pin, int flags, int info[8], unsigned long long digest[8]);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Hard-decision decoding: packed hard bits, a binary symmetric channel and two bit-flipping decoders.
 *
 * Packed hard bits.  `bits` is uint32 [rows][W] with W = ceil(F / 32): frame f of row n is bit f % 32 of word [n][f / 32].  The bits
 * of frames >= F in the last word of a row are padding: every producer below writes them as 0, every consumer ignores them.
 *   bldpc_hard_pack       bit = Channel_Out[n][f] < 0, the layered decoders' hard-bit rule (-0.0f and NaN give 0)
 *   bldpc_hard_pack_int   bit = CodeWord[n][f] != 0
 *   bldpc_hard_unpack     D[n][f] = the bit, int32 0 or 1
 * The device forms are asynchronous on `stream`; each has a _host statement over host arrays.
 *
 * Binary symmetric channel.  bits[n][f] = CodeWord[n][f] (NULL: the all-zero word) xor (u < p), u the draw f * N + n of the
 * RandomModule stream `seed` (frame outer, bit inner, one draw per bit, a float compare).  seed is advanced by N * F draws, as the
 * AWGN calls advance theirs.  BLDPC_EINVAL: p not finite or outside [0, 0.5], a seed state outside [0, modulus).
 *
 * Bit flipping.  Per frame: r[N] the received bits, x = r; d_v the column weight of v; s_c the XOR of x_v over check row c (rows and
 * their variables as in bldpc_decode_layered).  Iteration k = 1 .. max_iter:
 *   1. if every s_c is 0 nothing flips;
 *   2. otherwise, with u_v the number of unsatisfied checks of v and e_v = x_v xor r_v, all flips are decided from the same s and
 *      applied together:
 *        BLDPC_BF_THRESHOLD  flip v iff 2 u_v + e_v > d_v
 *        BLDPC_BF_GRADIENT   flip every v with E_v = u_v + e_v equal to the maximum of E over the N variables of the frame
 *   3. s is recomputed; the flag is "every s_c is 0".
 * BLDPC_EXIT_PER_FRAME: a frame stops after the first iteration that leaves its flag set, iters[f] is that k (a clean word: 1).
 * BLDPC_EXIT_FIXED: max_iter iterations, iters[f] = max_iter when iters is given.  A converged frame never flips again, so both
 * modes return the same D, Dbits and flags.  BLDPC_EXIT_BATCH_GLOBAL is refused.
 *   D      int32 [N+1][F], row N the flag (what bldpc_statistic and bldpc_syndrome take), or NULL
 *   Dbits  uint32 [N+1][W] packed, row N the flags, or NULL; at least one of the two
 * BLDPC_EINVAL: unknown rule or mode, max_iter < 1, F <= 0, null input, both outputs null, iters NULL with per-frame exit.
 * BLDPC_EUNSUPPORTED (kept with the code object, the same text at every call): a code built from an address table; a code whose
 * 32-frame state, 4 (N + M) bytes, exceeds the LDS a workgroup may use (there is no workspace tier).  Block rows of weight 1 and
 * block columns of weight 0 are taken.  The device call is asynchronous on `stream` and allocates nothing once its scratch has grown;
 * the _host form is the definition (plain C++, one frame at a time, at most 16 threads).
 *
 * bldpc_bitflip_info / bldpc_bitflip_plan_host: info[4] = LDS bytes of a workgroup of k_bf, threads, frames per workgroup, 0; the
 * first for a code object without a launch, the second without a device.  A code fits when info[0] <= 162816. */
#define BLDPC_BF_THRESHOLD 0
#define BLDPC_BF_GRADIENT 1
int bldpc_hard_pack(const float *Channel_Out, int N, int F, unsigned *bits, void *stream);
int bldpc_hard_pack_int(const int *CodeWord, int N, int F, unsigned *bits, void *stream);
int bldpc_hard_unpack(const unsigned *bits, int rows, int F, int *D, void *stream);
int bldpc_hard_pack_host(const float *Channel_Out, int N, int F, unsigned *bits);
int bldpc_hard_pack_int_host(const int *CodeWord, int N, int F, unsigned *bits);
int bldpc_hard_unpack_host(const unsigned *bits, int rows, int F, int *D);
int bldpc_bsc_channel_device(int seed[3], float p, const int *CodeWord, int N, int F, unsigned *bits, void *stream);
int bldpc_bsc_channel_host(int seed[3], float p, const int *CodeWord, int N, int F, unsigned *bits);
int bldpc_decode_bitflip(bldpc_code *code, const unsigned *bits_in, int F, int max_iter, int rule, int exit_mode, int *D, unsigned *Dbits,
                         int *iters, void *stream);
int bldpc_decode_bitflip_host(int J, int L, int Z, const int *H, const unsigned *bits_in, int F, int max_iter, int rule, int exit_mode, int *D,
                              unsigned *Dbits, int *iters);
int bldpc_bitflip_info(bldpc_code *code, int info[4]);
int bldpc_bitflip_plan_host(int J, int L, int Z, const int *H, int info[4]);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Erasure decoding: a third value on the packed rung, a binary erasure channel, a parallel peeling decoder, rate matching and
 * statistics on packed words.
 *
 * Erased words.  Two packed arrays of the layout above: `bits` uint32 [rows][W] and `erased` of the same shape, 1 = erased.  The value
 * bit at an erased position carries no meaning: every producer below writes it as 0, every consumer ignores it.  Padding bits of both
 * arrays are written as 0 and ignored on input.
 *
 * Binary erasure channel.  erased[n][f] = (u < p), u the draw f * N + n of the RandomModule stream `seed`: the BSC's indexing, one draw
 * per bit, the same float compare, so with equal seed and p the mask is the BSC's flip mask.  bits = CodeWord & ~erased (NULL: the
 * all-zero word).  seed is advanced by N * F draws.  BLDPC_EINVAL: p not finite or outside [0, 1], a seed state outside [0, modulus).
 *
 * Peeling.  Per frame, rows and their variables as in bldpc_decode_bitflip: x = bits_in & ~erased_in, er = erased_in.  Iteration
 * k = 1 .. max_iter decides everything from the state at its start and applies it together:
 *   1. for every check row c: n_c = the number of erased variables of c, a_c = the XOR of x_v over the known variables of c;
 *   2. an erased variable v is resolved iff at least one of its checks has n_c == 1; it becomes known with x_v = the OR of a_c over
 *      those checks (on a consistent word they agree; the OR defines the result when the known bits are not from a codeword);
 *   3. the iteration is productive for the frame iff it resolved at least one variable.  Once an iteration is unproductive every
 *      later one is too, and an implementation may stop there.
 *   Dbits  uint32 [N+1][W]: rows 0 .. N-1 hold x, with 0 at positions still erased; row N is the flag "no erasure left and every check
 *          sum of x zero"; or NULL
 *   Ebits  uint32 [N][W], the residual mask, or NULL
 *   D      int32 [N+1][F], the unpacked Dbits (what bldpc_statistic and bldpc_syndrome take), or NULL
 *   iters  int32 [F] or NULL: the index of the last productive iteration of frame f, 0 when there was none (a frame without erasures,
 *          a frame that is stuck from the start)
 * There is no exit mode: peeling is idempotent after it stalls, so a fixed count and a per-frame exit return the same words.
 * BLDPC_EINVAL: a null input, F <= 0, max_iter < 1, all of D, Dbits and Ebits null.  BLDPC_EUNSUPPORTED (kept with the code object, the
 * same text at every call): a code built from an address table; a code whose 32-frame state, 4 (2 N + M) bytes, exceeds the LDS a
 * workgroup may use (there is no workspace tier).  Block rows of weight 1 and block columns of weight 0, 1 and 16 are taken.  The device
 * call is asynchronous on `stream` and allocates nothing once its scratch has grown; the _host form is the definition (plain C++, one
 * frame at a time, at most 16 threads).
 *
 * bldpc_erasure_info / bldpc_erasure_plan_host: info[4] = LDS bytes of a workgroup of k_er, threads, frames per workgroup (32), 0; the
 * first for a code object without a launch, the second without a device.  A code fits when info[0] <= 162816.
 *
 * Rate matching on packed words, for linear and circular profiles.  bldpc_rm_select_bits: tx[e] = bits[tx_pos[e]], [N][W] -> [E][W]
 * (bit for bit bldpc_hard_pack_int of bldpc_rm_select of the unpacked words).  bldpc_rm_recover_bits, [E][W] -> [N][W]: a shortened
 * position is known 0 (erased 0, bits 0); a punctured or otherwise unsent position is erased (erased 1, bits 0); a position sent once
 * or several times (the laps of a circular buffer) is known iff any copy arrived unerased, with the value of the first unerased copy in
 * transmission order.  rx_erased == NULL: nothing was erased.
 *
 * Statistics on packed words.  bldpc_statistic_bits accumulates the five counters of bldpc_statistic_per_frame, with the values that
 * call gives on the unpacked D had every position still erased been replaced by the complement of the sent bit: an unresolved bit is
 * a bit error.  Row N of Dbits is the flag.  Ebits == NULL: none erased; CodeWordBits == NULL: the all-zero word; iters == NULL: nothing
 * is added to Total_Iteration; length == 0: the code's K, as bldpc_statistic.  The _host form takes N in place of the code object and a
 * length in [1, N]. */
int bldpc_bec_channel_device(int seed[3], float p, const int *CodeWord, int N, int F, unsigned *bits, unsigned *erased, void *stream);
int bldpc_bec_channel_host(int seed[3], float p, const int *CodeWord, int N, int F, unsigned *bits, unsigned *erased);
int bldpc_decode_erasure(bldpc_code *code, const unsigned *bits_in, const unsigned *erased_in, int F, int max_iter, int *D, unsigned *Dbits,
                         unsigned *Ebits, int *iters, void *stream);
int bldpc_decode_erasure_host(int J, int L, int Z, const int *H, const unsigned *bits_in, const unsigned *erased_in, int F, int max_iter, int *D,
                              unsigned *Dbits, unsigned *Ebits, int *iters);
int bldpc_erasure_info(bldpc_code *code, int info[4]);
int bldpc_erasure_plan_host(int J, int L, int Z, const int *H, int info[4]);
int bldpc_rm_select_bits(const bldpc_rm *rm, const unsigned *bits, int F, unsigned *tx, void *stream);
int bldpc_rm_recover_bits(const bldpc_rm *rm, const unsigned *rx_bits, const unsigned *rx_erased, int F, unsigned *bits, unsigned *erased,
                          void *stream);
int bldpc_rm_select_bits_host(const bldpc_rm *rm, const unsigned *bits, int F, unsigned *tx);
int bldpc_rm_recover_bits_host(const bldpc_rm *rm, const unsigned *rx_bits, const unsigned *rx_erased, int F, unsigned *bits, unsigned *erased);
int bldpc_statistic_bits(const bldpc_code *code, const unsigned *Dbits, const unsigned *Ebits, const unsigned *CodeWordBits, int F, int length,
                         const int *iters, long long *counters, void *stream);
int bldpc_statistic_bits_host(int N, const unsigned *Dbits, const unsigned *Ebits, const unsigned *CodeWordBits, int F, int length,
                              const int *iters, long long *counters);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Erasure decoding by elimination: the maximum-likelihood decoder of the binary erasure channel.  Peeling stops at the first
 * stopping set; what is left is a linear system over GF(2), and this call solves it.  Layouts are those of "erasure decoding".
 *   bits_in, erased_in  uint32 [N][W]; value bits under an erasure and padding bits are ignored
 *   Dbits   uint32 [N+1][W], row N the flag "nothing erased and every check sum zero", or NULL
 *   Ebits   uint32 [N][W], the residual mask, or NULL
 *   D       int32 [N+1][F], the unpacked Dbits, or NULL
 *   status, rank  int32 [F] each, or NULL
 * Outputs must not overlap inputs.  The first N rows of a peeling Dbits together with its Ebits are a valid input pair: that is the
 * intended use.
 *
 * Per frame, independent of any elimination order: x = bits_in & ~erased_in, E the set of erased positions, e = |E|.  One equation per
 * check row c: the XOR of the unknowns x_v, v in E and in the row, equals a_c, the XOR of the row's known bits.
 *   BLDPC_ML_NONE          e == 0: x, nothing erased, rank 0
 *   BLDPC_ML_SKIPPED       e > max_erased: as the input (x, E), flag 0, rank -1
 *   BLDPC_ML_INCONSISTENT  the system has no solution (the known bits are no part of a codeword): as the input, flag 0, rank = the rank
 *                          of the coefficient matrix
 *   BLDPC_ML_SOLVED        rank == e: every unknown becomes known
 *   BLDPC_ML_PARTIAL       rank < e and some unknown has the same value in every solution
 *   BLDPC_ML_STUCK         rank < e and no unknown has the same value in every solution
 * In the three consistent cases an unknown is determined iff it has the same value in every solution (its unit vector is in the row
 * space of the coefficient matrix; in reduced row echelon form it is a pivot column whose row has no other coefficient).  Determined
 * unknowns become known with that value; the rest stay erased with value bit 0.  A row with one erasure determines it, so on a word
 * whose known bits come from a codeword the call gives what peeling followed by the call gives, and never less than peeling.  On an
 * inconsistent word peeling's OR rule and this call differ on purpose: this call leaves such a word as it came.
 * max_erased == 0 means M (with more unknowns than equations nothing is solved whole); any value in [1, N] is allowed.
 *
 * The device call: a list pass counts e per frame and lists the frames with 0 < e <= max_erased; persistent workgroups of k_er_ml take
 * one listed frame each, build its augmented matrix (M rows of wpr = ceil((max_erased + 1) / 32) words, the right-hand side in bit e)
 * and reduce it; a last pass writes the flag row.  tier: BLDPC_ML_LDS keeps the matrix in LDS (it fits when 4 M wpr bytes, two
 * bitmaps of 4 ceil(N / 32) bytes and the list of erased positions, 4 max_erased bytes, are at most 162816 bytes);
 * BLDPC_ML_WORKSPACE keeps it in a global slot owned by the workgroup, min(compute units, F, floor(1 GiB / matrix bytes)) slots a
 * call; BLDPC_ML_AUTO takes LDS when it fits.  bldpc_last_kernel names the tier that ran: "k_er_ml" or "k_er_ml_ws".  Asynchronous
 * on `stream`; allocates nothing once its scratch has grown.
 * BLDPC_EINVAL: a null input, F <= 0, max_erased outside [0, N], an unknown tier, all of D, Dbits and Ebits null.
 * BLDPC_EUNSUPPORTED: a code built from an address table; M above 65536; bitmaps and list above the LDS bound; BLDPC_ML_LDS when the
 * matrix does not fit (decided at the call: it depends on max_erased); a workspace of which not even one slot fits in 1 GiB.
 * The _host form is the definition (plain C++, one frame at a time, at most 16 threads) and has no size bound beyond max_erased.
 *
 * bldpc_erasure_ml_info / bldpc_erasure_ml_plan_host: info[4] = matrix bytes of a workgroup, threads, the tier taken (-1 when
 * refused), workspace slots at F = 65536 (0 on the LDS tier); the second without a device, for the 256 compute units of an MI355X. */
#define BLDPC_ML_NONE 0
#define BLDPC_ML_SOLVED 1
#define BLDPC_ML_PARTIAL 2
#define BLDPC_ML_STUCK 3
#define BLDPC_ML_INCONSISTENT 4
#define BLDPC_ML_SKIPPED 5
#define BLDPC_ML_AUTO 0
#define BLDPC_ML_LDS 1
#define BLDPC_ML_WORKSPACE 2
int bldpc_decode_erasure_ml(bldpc_code *code, const unsigned *bits_in, const unsigned *erased_in, int F, int max_erased, int tier, int *D,
                            unsigned *Dbits, unsigned *Ebits, int *status, int *rank, void *stream);
int bldpc_decode_erasure_ml_host(int J, int L, int Z, const int *H, const unsigned *bits_in, const unsigned *erased_in, int F, int max_erased,
                                 int *D, unsigned *Dbits, unsigned *Ebits, int *status, int *rank);
int bldpc_erasure_ml_info(bldpc_code *code, int max_erased, int tier, int info[4]);
int bldpc_erasure_ml_plan_host(int J, int L, int Z, const int *H, int max_erased, int tier, int info[4]);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Ordered-statistics reprocessing of order 0 (OSD-0, "BP + OSD"): what the soft decoders lack after belief propagation.  A frame
 * that ends with a non-zero syndrome usually has nearly all of its a-posteriori values right and the few wrong ones among the least
 * reliable; this call trusts the most reliable independent positions and re-derives the rest from the parity checks, so it always
 * returns a codeword.  It is the soft counterpart of "erasure decoding by elimination".
 *   app      float [N][F]: any decoder's app, or a channel array (a quantised app converted to float, which is exact)
 *   D_in     int32 [N+1][F] or NULL.  Only the frames whose flag, row N, is 0 are processed; with NULL every frame is.  A kept frame
 *            is copied from D_in unchanged (all N+1 rows, whatever they hold), flips = -1, scanned = 0
 *   D        int32 [N+1][F]; may be D_in itself (any other overlap is undefined).  A processed frame gets c in rows 0 .. N-1 and flag 1
 *   flips, scanned  int32 [F] each, or NULL
 *
 * Per processed frame f, independent of any elimination order:
 *   y[v] = app[v][f] < 0, so -0.0f gives 0, as in the decoders.
 *   The reliability of v is key[v], the bit pattern of |app[v][f]| as uint32.  NaN is undefined, as elsewhere.
 *   The order is the positions ascending by (key[v], v): ties in the value go to the lower position, so the order is total.
 *   The least reliable basis B: walk the positions in that order; a position joins B iff its column of H is linearly independent
 *   over GF(2) of the columns already in B.  |B| = rank(H); a weight-0 column never joins; a rank-deficient H is fine.
 *   scanned is the 1-based place in the order of the last position that joined (0 when rank(H) = 0).
 *   The result c has c[v] = y[v] outside B, and on B it is the unique solution of H c = 0: c = y xor e with e supported on B and
 *   H_B e_B = H y, which is always consistent because B spans the column space.  By matroid duality the complement of B holds the
 *   most reliable independent positions, so this is OSD-0.
 *   flips is the weight of e.
 *
 * The device call: a list pass puts the frames with flag 0 on a list through a counter and copies the kept frames when D != D_in;
 * persistent workgroups of k_osd take one listed frame each: gather the frame's column of app, sort the 64-bit keys (key << 32) | v in
 * LDS (bitonic, over the next power of two P >= N, padded with all-ones keys), then eliminate with one barrier per position visited.
 * The columns of H are not stored; the workgroup keeps the M x M record T of the row operations and the reduced syndrome T (H y) as
 * one more bit per row, wpr = M / 32 + 1 words a row, and forms the reduced column of a position from T and the position's checks.
 * It stops after rank(H) pivots (the rank is the one of the code's generator, bldpc_encoder_info, built on first use).
 * tier: BLDPC_ML_LDS keeps the record in LDS: it fits when 4 M wpr bytes, the keys, 8 P bytes, two bitmaps of 4 ceil(N / 32) bytes and
 * 4 M bytes of pivot positions are at most 162816 bytes.  BLDPC_ML_WORKSPACE keeps the record in a global slot owned by the workgroup,
 * min(compute units, F, floor(1 GiB / record bytes)) slots a call, and the rest in LDS.  BLDPC_ML_AUTO takes LDS when it fits.
 * bldpc_last_kernel names the tier that ran: "k_osd" or "k_osd_ws".  Asynchronous on `stream`; allocates nothing once its scratch has
 * grown.
 * BLDPC_EINVAL: a null code, app or D, F <= 0, an unknown tier.
 * BLDPC_EUNSUPPORTED: a code built from an address table; M above 65536; keys, bitmaps and pivot positions above the LDS bound on
 * either tier (8 P + 8 ceil(N / 32) + 4 M > 162816: PON_LDPC and J15_L30_Z1280 among the shipped matrices); BLDPC_ML_LDS when the
 * record does not fit beside them; a workspace of which not even one slot fits in 1 GiB.
 * The _host form is the definition (plain C++, one frame at a time, at most 16 threads) and has no size bound.
 *
 * bldpc_osd_info / bldpc_osd_plan_host: info[4] = LDS bytes of a workgroup on the tier taken (of the LDS tier when refused), threads,
 * the tier taken (-1 when refused), workspace slots at F = 65536 (0 on the LDS tier); the second without a device, for the 256
 * compute units of an MI355X. */
int bldpc_decode_osd(bldpc_code *code, const float *app, const int *D_in, int F, int tier, int *D, int *flips, int *scanned, void *stream);
int bldpc_decode_osd_host(int J, int L, int Z, const int *H, const float *app, const int *D_in, int F, int *D, int *flips, int *scanned);
int bldpc_osd_info(bldpc_code *code, int tier, int info[4]);
int bldpc_osd_plan_host(int J, int L, int Z, const int *H, int tier, int info[4]);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Reprocessing of order 1 and 2 (OSD-1, and the "combination sweep" OSD-CS): order 0 trusts every position outside B; these calls
 * also try the words in which one trusted position, or a pair among the least reliable trusted positions, is flipped, and keep the
 * candidate with the least soft metric.  app, D_in, D, flips, scanned, the order of the positions ("place": a position's index in
 * it), the basis B, y, scanned and the kept frames are exactly those of bldpc_decode_osd.
 *   order    0, 1 or 2;  lambda >= 0, read at order 2 only
 *   picked   int32 [2][F] or NULL: the positions (not places) of the set S chosen, in ascending place, -1 where absent
 *   metric   float [F] or NULL: the metric of the candidate chosen; a NaN has an unspecified payload
 * A kept frame gets flips = -1, scanned = 0, picked = -1, -1 and leaves metric unwritten.
 *
 * Per processed frame f: B[0 .. rank-1] are the basis positions in the order they joined, w[v] the float whose bits are
 * bits(app[v][f]) & 0x7fffffff.
 *   A candidate is a set S of at most `order` positions outside B.  Its error pattern e has e[v] = 1 on S, and on B it is the unique
 *   solution of H_B e_B = H y xor H_S 1 (always consistent, because B spans the column space); its word is c = y xor e, a codeword.
 *   Its metric, in fp32: m = +0.0f; for k = 0 .. rank-1 in that order m += w[B[k]] where e[B[k]] = 1; then m += w[v] for the
 *   positions of S in ascending place.  No term is skipped or reassociated and there is no multiply to fuse.  Every term is
 *   non-negative, so m is +0.0, positive, +inf or NaN and its bit pattern orders as an unsigned integer; a NaN of any payload
 *   compares as 0x7fffffff.
 *   order 0: the empty set only; D, flips and scanned are those of bldpc_decode_osd, bit for bit.
 *   order 1: also every single position outside B, the dependent positions before `scanned` included: N - rank of them.
 *   order 2: also every pair among the first min(lambda, N - rank) positions outside B in ascending place; lambda = 0 is order 1.
 *   The result is the candidate with the least triple (metric bits, place of the first position of S + 1, place of the second + 1),
 *   a component being 0 where S has no such position: an exact tie stays with order 0, then goes to the single of lowest place, then
 *   to pairs.  The triple is a total order, so the result does not depend on who evaluates what first.
 *   D gets the word and flag 1; flips is the weight of the whole e, S included.
 *
 * The device call is the one of bldpc_decode_osd up to the last pivot (the same frame body, instantiated with the search), with one
 * addition: the thread that owns a pivot's row puts 0x80000000 | row into the lower half of the pivot's sort key, whose upper half
 * is bits(w) already.  The sorted keys are then the pivot list in joining order with its weights, the basis bitmap (bit 31) and the
 * positions outside B at once, so the search takes no LDS beyond k_osd's and the plan, the tier and the refusals of a shape are
 * those of bldpc_osd_info at every order.  One wave per candidate: 64 places a step, a lane whose place is a pivot XORs the reduced
 * columns of S at its row (from T and the checks of the positions, as the elimination does) into its syndrome bit, a ballot gives
 * the ones in joining order and the fp32 sum runs over them; a partial sum above the wave's best metric ends the candidate, which
 * loses nothing because every term is non-negative; for the same reason a wave stops at the first place whose weight alone, or whose
 * weight with that of the pair's first position, is above its best metric (the weights ascend with the place).  Wave i of the workgroup takes the places i, i + waves, ... outside B as
 * singles and each with the later places below the lambda-th as pairs; the least 64-bit key (metric bits, place + 1, place + 1 in
 * 16 bits each) of the waves goes through one LDS atomicMin per wave, and e of the winner is formed once.
 * bldpc_last_kernel names "k_osd_w" or "k_osd_w_ws".  Asynchronous on `stream`; allocates nothing once its scratch has grown.
 * BLDPC_EINVAL: what bldpc_decode_osd refuses, an order outside 0 .. 2, a negative lambda.
 * BLDPC_EUNSUPPORTED: what bldpc_osd_info refuses.
 * The _host form is the definition (plain C++, one frame at a time, at most 16 threads) and has no size bound.
 *
 * bldpc_osd_w_info / bldpc_osd_w_plan_host: info[4] as bldpc_osd_info gives it, for the order asked. */
int bldpc_decode_osd_w(bldpc_code *code, const float *app, const int *D_in, int F, int tier, int order, int lambda, int *D, int *flips,
                       int *scanned, int *picked, float *metric, void *stream);
int bldpc_decode_osd_w_host(int J, int L, int Z, const int *H, const float *app, const int *D_in, int F, int order, int lambda, int *D,
                            int *flips, int *scanned, int *picked, float *metric);
int bldpc_osd_w_info(bldpc_code *code, int tier, int order, int info[4]);
int bldpc_osd_w_plan_host(int J, int L, int Z, const int *H, int tier, int order, int info[4]);

const char *bldpc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
