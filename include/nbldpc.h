/*
 * nbldpc.h -- C ABI of the MI355X-native GF(q) non-binary LDPC EMS decoder.
 *
 * Drop-in boundary for the reference's NB hot path (gsw4869/CUDA_LDPC, directory
 * myNBLDPC/): Decoding_EMS (include/LDPC_Decoder.h:13, src/LDPC_Decoder.cpp:172-317)
 * and its GPU twin Decoding_EMS_GPU (include/Decode_GPU.cuh:17).  Canonical
 * semantics = the reference's CPU decoder (the only path of the reference whose float
 * operation order is defined); results are bit-identical to it.
 *
 * The reference decodes ONE frame per call out of pointer-rich VN/CN objects; here a
 * call decodes a batch of B independent frames from flat arrays:
 *   L_ch          float [B][N][q-1]   element k-1 <-> field element k (element 0 has LLR 0),
 *                                     what Demodulate leaves in VN[i].L_ch (LDPC_Decoder.cpp:139-157)
 *   DecodeOutput  int32 [B][N]        hard symbols (Decoding_EMS argument of the same name)
 *   iter_number   int32 [B]           as the reference leaves it: decremented once on success
 *                                     (LDPC_Decoder.cpp:232-238), == maxIT on failure
 *   ok            int32 [B]           the reference's return value (1 = zero syndrome reached)
 * Graph arrays flatten VN[]/CN[] (include/struct.h:27-45), -1 padded:
 *   vn_weight[N], vn_linkCNs[N][dvmax], vn_linkCNs_GF[N][dvmax]
 *   cn_weight[M], cn_linkVNs[M][dcmax], cn_linkVNs_GF[M][dcmax]
 * All functions return NBLDPC_OK or a negative code; nbldpc_last_error() has the text.
 */
#ifndef CUDA_LDPC_AMD_NBLDPC_H
#define CUDA_LDPC_AMD_NBLDPC_H

#ifdef __cplusplus
extern "C" {
#endif

#define NBLDPC_OK 0
#define NBLDPC_EINVAL (-1)
#define NBLDPC_ENOMEM (-2)
#define NBLDPC_EHIP (-3)
#define NBLDPC_EIO (-4)
#define NBLDPC_EUNSUPPORTED (-5)

typedef struct nbldpc_code nbldpc_code;

/* Replaces Get_H (src/Simulation.cpp:347-467): "N M q / dvmax dcmax / N column weights / M row weights /
 * per VN (cn_1based, gf)*w / per CN (vn_1based, gf)*w".  Call with all arrays NULL to obtain
 * dims[0..4] = N, M, q, dvmax, dcmax, then again with arrays sized from them (host memory). */
int nbldpc_read_matrix(const char *path, int dims[5], int *vn_weight, int *vn_linkCNs, int *vn_linkCNs_GF, int *cn_weight,
                       int *cn_linkVNs, int *cn_linkVNs_GF);

/* Replaces GFInitial (src/GF.cpp:68-117): reads "Multiply Table" q*q, "Add Table" q*q, "Inverse Table" q. */
int nbldpc_gf_load(const char *path, int q, unsigned *TableMultiply, unsigned *TableAdd, unsigned *TableInverse);

/* The same tables computed from the primitive polynomial (e.g. 67 = x^6+x+1 for GF(64), first line of
 * GF/Arith.Table.GF.64.txt); polynomial-basis representation, add == XOR. */
int nbldpc_gf_generate(int q, unsigned primitive_poly, unsigned *TableMultiply, unsigned *TableAdd, unsigned *TableInverse);

/* Upload a code.  TableMultiply: host unsigned [q][q].  q a power of two, 4 <= q <= 256; column weights <= 8; row weights 2..64.
 * The fused kernels (one frame's message state inside one CU's LDS) take q in {16, 32, 64} (a message vector inside one wave, EMS
 * and trellis decoders) and q in {128, 256} (a vector over q/64 waves, EMS only) with row weights up to 6 (e.g.
 * BDS.576.288.GF.64.txt, LDPC_N96_K48_GF256_d1_exp.txt); every other code (Tanner_74_9_Z128_GF16.txt: row weight 21, 7.5 MB of
 * state; LDPC_N576_K480_GF256_exp.txt: row weight 12) is decoded by the workspace kernel (EMS only, same results, far slower).
 * nbldpc_tmm_decode_batch returns NBLDPC_EUNSUPPORTED where the trellis kernels do not apply.  A zero edge coefficient is
 * accepted for EMS (the reference reads its exponent-format files as field elements and decodes with the zeros in place); the
 * trellis decoders refuse such a code (the reference's GFInverse(0) exits). */
int nbldpc_code_create(int N, int M, int q, int dvmax, int dcmax, const int *vn_weight, const int *vn_linkCNs,
                       const int *vn_linkCNs_GF, const int *cn_weight, const int *cn_linkVNs, const int *cn_linkVNs_GF,
                       const unsigned *TableMultiply, nbldpc_code **code);
int nbldpc_code_destroy(nbldpc_code *code);

/* Name of the kernel the last decode call on this code launched (static string): "k_nb_ems2" = two frames in flight per workgroup,
 * "k_nb_ems" / "k_nb_ems_wide" one frame per workgroup (+ " (frames from a counter)": persistent workgroups), "k_nb_ems_hbm" the
 * workspace kernel, "k_nb_tmm…" the trellis decoders, "k_nb_qspa…" the FHT sum-product decoders.  The counterpart of bldpc_last_kernel (include/bldpc.h); the reference has no
 * equivalent -- its kernels are fixed at compile time (myNBLDPC/src/Decode_GPU.cu:138-356). */
const char *nbldpc_last_kernel(const nbldpc_code *code);

/* How many workgroups of this code's kernels the device holds at once, as nbldpc_code_create found it: info[0] k_nb_ems /
 * k_nb_ems_wide, info[1] k_nb_ems2, info[2] / info[3] k_nb_tmm flooding / layered; 0: no such kernel for this code (or the device
 * did not say).  A batch with more frames than that is decoded by persistent workgroups that take their frames from a counter.
 * The counterpart of bldpc_code_qc_info's persist_grid (include/bldpc.h). */
int nbldpc_code_grids(const nbldpc_code *code, int info[4]);

/* Replaces Decoding_EMS / Decoding_EMS_GPU for a batch (all pointers DEVICE memory).
 *   EMS_Nm, EMS_Nc   reference macros EMS_NM / EMS_NC (define.h:31-32)
 *   maxIT            reference macro maxIT (define.h:35)
 *   maxdc_cfg        reference macro maxdc (define.h:28), used by the `EMS_Nc == maxdc - 1` test
 *                    (LDPC_Decoder.cpp:294); pass 0 for the code's dcmax
 *   LLR     optional float [B][N][q-1]       VN[].LLR of the last executed iteration
 *   L_c2v   optional float [B][M][dcmax][q-1] CN[].L_c2v as the reference leaves it
 *   stream  hipStream_t; the call is asynchronous. */
int nbldpc_ems_decode_batch(nbldpc_code *code, const float *L_ch, int B, int EMS_Nm, int EMS_Nc, int maxIT, int maxdc_cfg,
                            int *DecodeOutput, int *iter_number, int *ok, float *LLR, float *L_c2v, void *stream);

/* Trellis min-max decoders for a batch of frames: Decoding_TMM (decoder_method 1, myNBLDPC/src/LDPC_Decoder.cpp:361-558,
 * flooding) and Decoding_layered_TMM (decoder_method 3, :560-702; layered != 0), called from decode_once_cpu/gpu
 * (src/Simulation.cpp:58-70, :132-143) with the same arguments as Decoding_EMS.  Same outputs and return convention as
 * nbldpc_ems_decode_batch (ok = 1: zero syndrome reached, iter_number already decremented).  Optional state outputs hold
 * the reference's VN[].LLR and CN[].L_c2v after the call with ALL q entries per vector (element 0 included):
 * LLR DEVICE float [B][N][q], L_c2v DEVICE float [B][M][dcmax][q]; NULL to skip.  The layered schedule visits the
 * rows in dependency levels (rows that share no variable node commute), which leaves every value and its order of
 * computation per variable as in the reference's row-by-row loop. */
int nbldpc_tmm_decode_batch(nbldpc_code *code, const float *L_ch, int B, int layered, int maxIT, int *DecodeOutput, int *iter_number,
                            int *ok, float *LLR, float *L_c2v, void *stream);

/* Replaces Demodulate, BPSK branch (src/LDPC_Decoder.cpp:132-157), on the device:
 * rx float [B][N*m] (m = log2 q, bit b of symbol s at s*m+b) -> L_ch float [B][N][q-1]. */
int nbldpc_demodulate_bpsk(const nbldpc_code *code, const float *rx, float sigma, int B, float *L_ch, void *stream);

/* The same two without a code object (Demodulate needs the dimensions only): N symbols of GF(q). */
int nbldpc_demodulate_bpsk_nq(int N, int q, const float *rx, float sigma, int B, float *L_ch, void *stream);
int nbldpc_demodulate_qam_nq(int N, int q, const float *rx, const float *constellation, float sigma, int B, float *L_ch, void *stream);

/* Device-side Statistic (src/Simulation.cpp:256-279) over a decoded batch: counters device int64[4],
 * ACCUMULATED: [0] num_Error_Frames [1] num_Error_Bits (symbol errors, sic) [2] Total_Iteration [3] frames ok.
 * CodeWord_sym: device int32 [N]. */
int nbldpc_statistic(const nbldpc_code *code, const int *DecodeOutput, const int *iter_number, const int *ok,
                     const int *CodeWord_sym, int B, long long *counters, void *stream);

/* Host input generator, bit-identical to the reference (BPSK, n_QAM 2): Modulate of the codeword bits
 * (src/main.cu:203-211, Constellation/BPSK.txt: bit 0 -> +1, bit 1 -> -1) + AWGNChannel_CPU
 * (src/LDPC_Encoder.cpp:41-68: four RandomModule draws per bit, cos branch).  rx: HOST float [N*m] for
 * ONE frame; seed[3] advanced in place. */
int nbldpc_awgn_channel_host(int seed[3], float sigma, const int *CodeWord_sym, int N, int m, float *rx);

/* Device-side input generator: the same stream for B consecutive frames.  Every (frame, bit) jumps the
 * three LCGs of RandomModule (src/LDPC_Encoder.cpp:70-79) ahead to its own first draw (draw 4*(b*N*m + i):
 * seed * a^k mod m), so the uniforms are the reference's exactly; the samples are then formed with the device's
 * logf / sqrtf / cos, which may differ from the host libm by an ulp on a small fraction of arguments.
 * CodeWord_sym: DEVICE int32 [N]; rx: DEVICE float [B][N*m]; seed[3] (host) is advanced by B whole frames exactly
 * like B calls of nbldpc_awgn_channel_host. */
int nbldpc_awgn_channel_device(int seed[3], float sigma, const int *CodeWord_sym, int N, int m, int B, float *rx, void *stream);

/* ---- QAM constellations (n_QAM != 2 branches; n_QAM = q: one constellation point per code symbol).  The reference's define.h:25
 * fixes n_QAM 2; these entry points are checked against the reference BUILT with n_QAM 64 and Constellation/GRAY_64QAM.txt
 * (oracle/_ref/nb_ref_qam64, fixtures tests/golden/nb_ref_qam64_*.npz): channel samples, L_ch and decode results bit for bit. ---- */

/* Replaces Get_CONSTELLATION (src/Simulation.cpp:313-338): n_points records "Point: <idx> Real: <x> Imag: <y>" ->
 * constellation HOST float [n_points][2] (Real, Image), indexed by the record's own idx. */
int nbldpc_read_constellation(const char *path, int n_points, float *constellation);

/* Modulate (src/LDPC_Encoder.cpp:18-28: symbol s -> CONSTELLATION[CodeWord_sym[s]]) + AWGNChannel_CPU with
 * len = Variablenode_num (:41-68: two draws for the Real part, two for the Image part, cos branch).
 * rx: HOST float [N][2] for ONE frame; seed[3] advanced in place. */
int nbldpc_awgn_channel_host_qam(int seed[3], float sigma, const int *CodeWord_sym, int N, const float *constellation, int n_points,
                                 float *rx);

/* The same for B consecutive frames on the device (LCG jump-ahead per symbol, device libm as nbldpc_awgn_channel_device).
 * CodeWord_sym: DEVICE int32 [N]; constellation: DEVICE float [q][2]; rx: DEVICE float [B][N][2]. */
int nbldpc_awgn_channel_device_qam(int seed[3], float sigma, const int *CodeWord_sym, int N, const float *constellation, int B, float *rx,
                                   void *stream);

/* Replaces Demodulate, n_QAM != 2 branch (src/LDPC_Decoder.cpp:160-169), on the device:
 * rx float [B][N][2], constellation DEVICE float [q][2] -> L_ch float [B][N][q-1]. */
int nbldpc_demodulate_qam(const nbldpc_code *code, const float *rx, const float *constellation, float sigma, int B, float *L_ch,
                          void *stream);

/* ---- AWGNChannel_CPU exactly as the reference declares it (src/LDPC_Encoder.cpp:41-68): noise added to a MODULATED frame,
 * whatever produced it -- len samples (bit_length for BPSK, Variablenode_num for n_QAM != 2), each a (Real, Image) pair with
 * two RandomModule draws per part.  tx / rx: HOST float [len][2], i.e. the memory of a CComplex array (include/struct.h:9-14).
 * nbldpc_awgn_channel_host / _host_qam above are this function composed with Modulate. */
int nbldpc_awgn_channel_host_sym(int seed[3], float sigma, const float *tx, int len, float *rx);

/* The same for B consecutive frames on the device (LCG jump-ahead per run of samples, device libm).  tx: DEVICE float [len][2];
 * rx: DEVICE float [B][len] holding the Real parts only when real_only != 0 (what nbldpc_demodulate_bpsk takes), else
 * DEVICE float [B][len][2] (nbldpc_demodulate_qam).  seed[3] (host) is advanced by B whole frames. */
int nbldpc_awgn_channel_device_sym(int seed[3], float sigma, const float *tx, int len, int B, int real_only, float *rx, void *stream);

/* RandomModule (src/LDPC_Encoder.cpp:70-79): one uniform draw, seed[3] advanced in place. */
float nbldpc_random_module(int seed[3]);

/* Advance the three LCGs of RandomModule (src/LDPC_Encoder.cpp:70-79) by `draws` calls: seed_i * a_i^draws mod m_i.  One frame
 * of AWGNChannel_CPU is 4 * len draws. */
int nbldpc_seed_jump(int seed[3], unsigned long long draws);

/* Per-frame symbol errors against the transmitted word (the count Statistic makes, src/Simulation.cpp:264-267):
 * DecodeOutput DEVICE int32 [B][N], CodeWord_sym DEVICE int32 [N] -> errs DEVICE int32 [B]. */
int nbldpc_frame_errors(const nbldpc_code *code, const int *DecodeOutput, const int *CodeWord_sym, int B, int *errs, void *stream);

/* sigma of a sweep point (src/main.cu:221-228). */
float nbldpc_sigma(float SNR, int snrtype, int n_QAM, float rate);

/* ---- encoder and syndrome check.  The reference sends one fixed CodeWord_sym that every frame shares (src/main.cu:190-212 copies
 * codeword_test.h).  These entry points encode real messages, one codeword per frame, for any code object (H as the decoders see it:
 * entry (r, v) of the M x N symbol matrix is the XOR of the coefficients of all edges (r, v); a coefficient 0 contributes nothing).
 *
 * Generator: Gauss-Jordan over GF(q) on the dense H, multiplication by TableMultiply[symbol][coefficient], addition XOR, pivot
 * columns searched from the right (N-1 down to 0), every pivot row normalised to 1.  The pivot columns are the parity positions, the
 * other K' = N - rank(H) columns the information set info_pos[K'] (ascending); information symbol k of a message goes to codeword
 * position info_pos[k].  Parity row r belongs to the r-th parity position in ascending order, par_pos[r], and
 *     c[par_pos[r]] = XOR_j TableMultiply[msg[j]][P[r][j]],     P uint8 [rank][K'].
 * For codes whose last M columns are invertible, info_pos = 0 .. K-1 with K = N - M.  TableMultiply must be a field table with XOR
 * addition (commutative, 1 the identity, distributive over XOR, associative, every nonzero element invertible): otherwise
 * NBLDPC_EUNSUPPORTED. ---- */

/* Host only (no device needed): the generator from the CN lists (as nbldpc_read_matrix returns them) and TableMultiply (host unsigned
 * [q][q]).  Sizes come back in *K_info and *rank; info_pos (int [K']) and P (rank * K' bytes) are filled when not NULL, so a call with
 * both NULL returns the sizes.  Dense elimination on up to 16 threads. */
int nbldpc_generator_host(int N, int M, int q, int dcmax, const int *cn_weight, const int *cn_linkVNs, const int *cn_linkVNs_GF,
                          const unsigned *TableMultiply, int *K_info, int *rank, int *info_pos, unsigned char *P);

/* K', rank and (when not NULL) info_pos[K'] of the code's generator.  The generator is built on the first call of this function,
 * nbldpc_encode or nbldpc_encode_random on the code object (from the copies of the CN lists and of TableMultiply that
 * nbldpc_code_create keeps), kept with it and freed by nbldpc_code_destroy. */
int nbldpc_encoder_info(nbldpc_code *code, int *K_info, int *rank, int *info_pos);

/* Systematic encoding of B messages on the device.
 *   msg           DEVICE int32 [B][K']  (in)  frame-outer; only the low m = log2 q bits of each entry are read
 *   CodeWord_sym  DEVICE int32 [B][N]   (out) H * c = 0 over GF(q), CodeWord_sym[b][info_pos[k]] = msg[b][k] & (q-1)
 * Asynchronous on `stream` (after the generator exists). */
int nbldpc_encode(nbldpc_code *code, const int *msg, int B, int *CodeWord_sym, void *stream);

/* The same with messages generated on the device by a counter-based rule, so that any frame can be drawn on its own.  With
 * m = log2 q, s = floor(64 / m) symbols per word and W = ceil(K' / s) words per frame, symbol k of global frame g = first_frame + b is
 *     (splitmix64(seed + g * W + k / s) >> (m * (k % s))) & (q - 1)          (uint64 arithmetic, wrapping)
 * with splitmix64 the function include/bldpc.h defines (the first output of SplitMix64 seeded with x).
 *   first_frame >= 0;  msg  optional DEVICE int32 [B][K'] (out): the messages, NULL to skip;  CodeWord_sym as nbldpc_encode. */
int nbldpc_encode_random(nbldpc_code *code, unsigned long long seed, long long first_frame, int B, int *msg, int *CodeWord_sym, void *stream);

/* Syndrome check of B words, the decoders' own check (src/LDPC_Decoder.cpp:219-230) on the low m bits of each symbol:
 * flag[b] = 1 iff H * d_b = 0 over GF(q), unsat[b] = the number of unsatisfied checks.
 *   DecodeOutput DEVICE int32 [B][N];  flag DEVICE int32 [B];  unsat DEVICE int32 [B] or NULL.  Asynchronous on `stream`. */
int nbldpc_syndrome(const nbldpc_code *code, const int *DecodeOutput, int B, int *flag, int *unsat, void *stream);

/* nbldpc_awgn_channel_device / _qam with one word per frame: CodeWord_sym DEVICE int32 [B][N], frame b sends row b.  Draws and seed
 * advance are those of the shared-word calls (frame b of the batch is frame b of the stream, whatever it sends).  The QAM form reads
 * the low log2 q bits of each symbol; constellation DEVICE float [q][2]. */
int nbldpc_awgn_channel_device_frames(int seed[3], float sigma, const int *CodeWord_sym, int N, int m, int B, float *rx, void *stream);
int nbldpc_awgn_channel_device_qam_frames(int seed[3], float sigma, const int *CodeWord_sym, int N, const float *constellation, int q, int B,
                                          float *rx, void *stream);

/* Block fading with receiver CSI (the model, the gain array float [B][N] and its generator: include/bldpc.h, "block fading").
 * nbldpc_fading_channel_device_qam_frames is nbldpc_awgn_channel_device_qam_frames in every respect -- four draws per symbol at
 * 4 (b*N + i), the q - 1 mask, the seed advance -- but for the transmitted part, which is (double)a * (double)constellation[2*sym + c]
 * with a = gain[b*N + i] instead of (double)constellation[2*sym + c]; a == 1.0f gives that call's bits.  It serves the binary QAM
 * chain (N := symbols per frame) and the GF(q) QAM chain alike.  gain: DEVICE float [B][N].  The _host form is the statement: host
 * pointers, the serial stream, host libm.  NBLDPC_EINVAL: a null pointer, N or B <= 0, q not a power of two, a seed outside its modulus. */
int nbldpc_fading_channel_device_qam_frames(int seed[3], float sigma, const int *CodeWord_sym, int N, const float *constellation, int q,
                                            const float *gain, int B, float *rx, void *stream);
int nbldpc_fading_channel_host_qam_frames(int seed[3], float sigma, const int *CodeWord_sym, int N, const float *constellation, int q,
                                          const float *gain, int B, float *rx);

/* nbldpc_demodulate_qam with CSI: with a = gain[b*N + s] the four products a*c0r, a*c0i, a*ckr, a*cki are formed first, each one fp32
 * multiplication, and then used in the expression of nbldpc_demodulate_qam, in its order, in place of c0r, c0i, ckr, cki:
 *     L_ch[b][s][k-1] = ((2*yr - c0r - ckr) * (ckr - c0r) + (2*yi - c0i - cki) * (cki - c0i)) / (2 * sigma * sigma)
 * a == 1.0f gives nbldpc_demodulate_qam's bits.  gain DEVICE float [B][N] (host for _host, which is the statement).  The GF(q) BPSK
 * path has no fading form.  Argument checks as nbldpc_demodulate_qam_nq, and gain != NULL. */
int nbldpc_demodulate_qam_fading_nq(int N, int q, const float *rx, const float *gain, const float *constellation, float sigma, int B,
                                    float *L_ch, void *stream);
int nbldpc_demodulate_qam_fading(const nbldpc_code *code, const float *rx, const float *gain, const float *constellation, float sigma, int B,
                                 float *L_ch, void *stream);
int nbldpc_demodulate_qam_fading_host(int N, int q, const float *rx, const float *gain, const float *constellation, float sigma, int B,
                                      float *L_ch);

/* nbldpc_statistic / nbldpc_frame_errors against one word per frame: CodeWord_sym DEVICE int32 [B][N]. */
int nbldpc_statistic_frames(const nbldpc_code *code, const int *DecodeOutput, const int *iter_number, const int *ok, const int *CodeWord_sym,
                            int B, long long *counters, void *stream);
int nbldpc_frame_errors_frames(const nbldpc_code *code, const int *DecodeOutput, const int *CodeWord_sym, int B, int *errs, void *stream);

/* ---- rate matching: shortening, puncturing and HARQ with symbol-LLR combining --------------------------------------------------
 *
 * Profile.  A profile is a bldpc_rm (include/bldpc.h, "rate matching" and "HARQ") whose positions are code SYMBOLS: made by
 * bldpc_rm_create or bldpc_rm_create_circular with N := the number of code symbols.  Same two lists, buffer (the Ncb positions neither
 * shortened nor punctured, ascending), k0, E, laps <= 8, tx_pos[e] = buffer[(k0 + e) mod Ncb], and the same rule for a position's
 * contributions: position n of rank r in the buffer is sent at e_0 = (r - k0) mod Ncb and again at e_0 + Ncb, e_0 + 2 Ncb, ... < E
 * (e_0 < e_1 < ...); a position with e_0 >= E is not reached.  No new object type and no new table: both halves are one library.
 *
 * Layout and LLR convention.  V = q - 1.  All arrays are frame-outer.  L_ch[b][n][k-1] = ln P(y | k) - ln P(y | 0), element 0
 * implicit at 0 -- what nbldpc_demodulate_qam computes, (|y - c0|^2 - |y - ck|^2) / 2 sigma^2 -- so the LLR vectors of independent
 * transmissions add entry by entry, and a symbol known to be 0 has every entry equal to -short_llr.
 *
 * select.   tx_sym[b][e] = CodeWord_sym[b][tx_pos[e]], int32 [B][N] -> [B][E].
 * recover.  Lrx float [B][E][V] -> L_ch float [B][N][V].  Entry k of a position with contributions is the 32 bits of Lrx[b][e_0][k],
 *           then + Lrx[b][e_1][k], and so on: fp32 additions in ascending e, not contracted, not reordered.  One contribution is a copy
 *           (-0.0f and NaN payloads survive).  A punctured position, or one not reached, gets all V entries 0x00000000; a shortened one
 *           gets all V entries -short_llr.
 * combine.  L_acc float [B][N][V] is read and written, for every frame with done[b] == 0 (every frame when done == NULL; done DEVICE
 *           int32 [B]).  A position with contributions becomes ((acc + Lrx[e_0]) + Lrx[e_1]) + ...; one without is left untouched; a
 *           shortened one becomes -short_llr.  A frame with done[b] != 0 keeps every bit of its N*V floats (they are not read either).
 * Fused receive.  Lrx[b][e][k-1] is not read but computed from the received sample of transmitted symbol e by the expression of the
 *           existing demodulator run at N := E (csrc/nbldpc_demod.hpp holds the two expressions; the demodulators and these calls both
 *           call them): the QAM form from rx float [B][E][2] and constellation DEVICE float [q][2] (nbldpc_demodulate_qam_nq), the BPSK
 *           form from rx float [B][E*m] (nbldpc_demodulate_bpsk_nq).  Each is, bit for bit, nbldpc_demodulate_*_nq(N := E) followed by
 *           nbldpc_rm_recover or nbldpc_rm_combine, in one launch whatever the number of laps and with no [B][E][V] array.
 * Channel.  None is added: a rate-matched transmission is nbldpc_rm_select followed by nbldpc_awgn_channel_device_qam_frames,
 *           nbldpc_fading_channel_device_qam_frames or nbldpc_awgn_channel_device_frames called with N := E.  Noise is drawn for the
 *           transmitted symbols only (4 E draws per frame over QAM, 4 E m over BPSK); a frame's draws depend neither on done nor on its
 *           batch mates.
 * Shortened encoding.  nbldpc_rm_encode_random applies the message rule of nbldpc_encode_random, forces to 0 every message symbol k
 *           whose info_pos[k] is a shortened position, and calls nbldpc_encode.  msg is required (DEVICE int32 [B][K'], the messages
 *           after the forcing).  NBLDPC_EINVAL when the profile's N differs from the code's or a shortened position is not in the
 *           information set; punctured positions play no part.
 * Host statements.  The _host calls are the words above in plain C++ on host pointers (csrc/nbldpc_rm_host.hpp, which a stand-alone
 *           program can compile without the device code); the fused _host calls are demodulate_*_nq_host(N := E) followed by
 *           recover_host / combine_host.  nbldpc_rm_force_shortened_host is the forcing step alone on msg HOST int32 [B][K'].
 * Checks.   NBLDPC_EINVAL, and nothing is launched: a null pointer (done excepted); B < 1; q not a power of two in 2 .. 256 (the code
 *           object of nbldpc_rm_encode_random has q >= 4); short_llr not finite or not > 0; sigma not > 0 (fused calls); N * V or E * V
 *           above 65535 * 1024 = 67 107 840 entries per frame (the launch indexes a frame's entries by gridDim.y blocks of 1024; B
 *           itself may be anything up to 2^31 - 1, offsets are 64-bit); for select E, and for nbldpc_rm_encode_random K', above
 *           65535 * 256 = 16 776 960 (gridDim.y blocks of 256; a profile's own limit on N and E, 65535 * 32, is lower).  The device calls
 *           are asynchronous on `stream`; nothing is allocated per call beyond the profile's table upload on its first device use.
 * Additions.  nbldpc_demodulate_qam_nq_host / _bpsk_nq_host below are not part of the rate matcher: they are the host statements of the
 *           two existing demodulators, added because the fused _host calls are defined as their composition with recover / combine. ---- */
typedef struct bldpc_rm bldpc_rm;

int nbldpc_rm_select(const bldpc_rm *rm, const int *CodeWord_sym, int B, int *tx_sym, void *stream);
int nbldpc_rm_recover(const bldpc_rm *rm, int q, const float *Lrx, int B, float short_llr, float *L_ch, void *stream);
int nbldpc_rm_combine(const bldpc_rm *rm, int q, const float *Lrx, int B, float short_llr, const int *done, float *L_acc, void *stream);
int nbldpc_rm_demodulate_qam_recover(const bldpc_rm *rm, int q, const float *rx, const float *constellation, float sigma, int B, float short_llr,
                                     float *L_ch, void *stream);
int nbldpc_rm_demodulate_qam_combine(const bldpc_rm *rm, int q, const float *rx, const float *constellation, float sigma, int B, float short_llr,
                                     const int *done, float *L_acc, void *stream);
int nbldpc_rm_demodulate_bpsk_recover(const bldpc_rm *rm, int q, const float *rx, float sigma, int B, float short_llr, float *L_ch, void *stream);
int nbldpc_rm_demodulate_bpsk_combine(const bldpc_rm *rm, int q, const float *rx, float sigma, int B, float short_llr, const int *done, float *L_acc,
                                      void *stream);
int nbldpc_rm_encode_random(nbldpc_code *code, const bldpc_rm *rm, unsigned long long seed, long long first_frame, int B, int *msg,
                            int *CodeWord_sym, void *stream);

int nbldpc_rm_select_host(const bldpc_rm *rm, const int *CodeWord_sym, int B, int *tx_sym);
int nbldpc_rm_recover_host(const bldpc_rm *rm, int q, const float *Lrx, int B, float short_llr, float *L_ch);
int nbldpc_rm_combine_host(const bldpc_rm *rm, int q, const float *Lrx, int B, float short_llr, const int *done, float *L_acc);
int nbldpc_rm_demodulate_qam_recover_host(const bldpc_rm *rm, int q, const float *rx, const float *constellation, float sigma, int B,
                                          float short_llr, float *L_ch);
int nbldpc_rm_demodulate_qam_combine_host(const bldpc_rm *rm, int q, const float *rx, const float *constellation, float sigma, int B,
                                          float short_llr, const int *done, float *L_acc);
int nbldpc_rm_demodulate_bpsk_recover_host(const bldpc_rm *rm, int q, const float *rx, float sigma, int B, float short_llr, float *L_ch);
int nbldpc_rm_demodulate_bpsk_combine_host(const bldpc_rm *rm, int q, const float *rx, float sigma, int B, float short_llr, const int *done,
                                           float *L_acc);
int nbldpc_rm_force_shortened_host(const bldpc_rm *rm, const int *info_pos, int K_info, int B, int *msg);

/* nbldpc_demodulate_qam_nq / _bpsk_nq as host statements (host pointers, the same expressions). */
int nbldpc_demodulate_qam_nq_host(int N, int q, const float *rx, const float *constellation, float sigma, int B, float *L_ch);
int nbldpc_demodulate_bpsk_nq_host(int N, int q, const float *rx, float sigma, int B, float *L_ch);

/* ---- FHT sum-product (QSPA): belief propagation proper over GF(2^m), the check node in the Walsh-Hadamard domain ---------------
 *
 * The reference has no such decoder (its decoder_method stops at 3; 2, "log-QSPA", is max-log).  This one is ours, and the host
 * statement nbldpc_qspa_decode_host, the words below in serial C++ (csrc/nbldpc_qspa_host.hpp), is its definition: the kernel equals
 * it bit for bit.  Every arithmetic step is one IEEE fp32 operation (+, -, *, /, compare), never contracted, in the order given;
 * nothing calls expf, logf or another library transcendental (csrc/nbldpc_qspa_math.hpp holds the expressions both sides call).
 *
 * Input.  L_ch float [B][N][q-1] as every decoder here takes it: x_0 = 0, x_k = L_ch[k-1] = ln P(k) / P(0).  Any finite values,
 * the +-1e4 and +0.0 of the rate matcher included; NaN and infinities are not inputs.
 * Probability vectors.  q fp32 entries, the largest exactly 1, none below kQspaFloor = 2^-40:
 *     norm(v)[a] = max(v[a] / max(v), 2^-40)                  max(v): the largest entry (order-independent), the division IEEE.
 * A product of two such vectors has a maximum of at least 2^-80, so no vector underflows to zero.
 * Channel vector.  p[a] = max(qspa_exp(x_a - max_a x_a), 2^-40), where qspa_exp(x) for x <= 0 is: 0 for x < -87 (or not ordered);
 *     else n = rintf(x * 0x1.715476p+0f), r = (x - n * 0x1.62e4p-1f) - n * 0x1.7f7d1cp-20f,
 *     poly = ((((((0x1.6d4932p-10f r + 0x1.12107cp-7f) r + 0x1.5554e4p-5f) r + 0x1.5554d8p-3f) r + 0x1p-1f) r + 1) r + 1),
 *     qspa_exp = poly * 2^n, the power of two built from its exponent bits.  qspa_exp(0) == 1; every result is 0 or normal.
 * Schedule.  Flooding, with the loop of Decoding_EMS (LDPC_Decoder.cpp:197-238).  All c2v start as all ones.  Iteration
 *     iter_number = 1, 2, ...: for every variable app = p, then for its edges d ascending app = norm(app * c2v_d); the decision is
 *     the first index of app's maximum; then the GF(q) syndrome over all rows, XOR_t TableMultiply[decision][h_t].  Zero syndrome:
 *     ok = 1, iter_number - 1 is reported, the frame is done.  Otherwise the messages below are formed, and after maxIT iterations
 *     ok = 0, iter_number = maxIT, DecodeOutput holds the last decision.
 * Variable to check.  v2c_d = p, then for d' ascending, d' != d: v2c_d = norm(v2c_d * c2v_d').
 * Check node.  For the edge in slot t of a row, coefficient h: u[TableMultiply[h][a]] = v2c[a]; W = FHT(u); U_t = W / W[0] entry by
 *     entry (U_t[0] == 1).  FHT: log2 q stages with strides 1, 2, 4, ... in that order; in a stage every pair (i, i + stride) with
 *     bit `stride` of i clear becomes (lo + hi, lo - hi).  Over the row's slots in order: F_0 = U_0, F_t = F_{t-1} * U_t;
 *     B_{w-1} = U_{w-1}, B_t = U_t * B_{t+1}; out_0 = B_1, out_{w-1} = F_{w-2}, else out_t = F_{t-1} * B_{t+1} (a row of weight 2
 *     passes the other edge's U through).  wv = max(FHT(out_t), 0), unscaled (norm removes the 1/q); c[a] = wv[TableMultiply[h][a]];
 *     c2v_t = norm(c), or all ones if max(c) == 0.
 * Outputs.  DecodeOutput, iter_number, ok as nbldpc_ems_decode_batch.  Optional APP float [B][N][q]: app of the last executed
 *     iteration; optional c2v float [B][M][dcmax][q]: the check-to-variable vectors after the call (those the last APP was formed
 *     from when ok = 1, those of iteration maxIT when ok = 0); slots beyond a row's weight hold the initial ones.  All q entries.
 * Refusals.  NBLDPC_EINVAL: a null pointer (APP and c2v excepted), B < 1, maxIT < 1, a graph whose two views differ.
 *     NBLDPC_EUNSUPPORTED: an edge coefficient 0 (the permutation would not be one; as nbldpc_tmm_decode_batch refuses it); q not a
 *     power of two with 4 <= q <= 256; and, nbldpc_qspa_decode_batch only, a code whose frame state exceeds the kernel's LDS:
 *         4 (N q + M dcmax q) + 4 (N + 4) + q^2  <=  159 * 1024 bytes
 *     (p, one message array reused in place, decisions and flag, TableMultiply as bytes).  BDS.576.288.GF.64.txt takes 78 224 bytes;
 *     Tanner_74_9_Z128_GF16.txt and LDPC_N576_K480_GF256_exp.txt do not fit.  Nothing is launched on a refusal.  A code
 *     that does not fit is decoded by the workspace tier below (nbldpc_qspa_ws_decode_batch), never by this call.
 * nbldpc_qspa_decode_batch: all pointers DEVICE memory, asynchronous on `stream`, return codes as nbldpc_ems_decode_batch; one
 *     workgroup per frame (k_nb_qspa in nbldpc_last_kernel).  nbldpc_qspa_decode_host: HOST pointers, the node arrays and
 *     TableMultiply of nbldpc_code_create, serial.  nbldpc_qspa_exp_host: y[i] = qspa_exp(x[i]), for the tests. ---- */
int nbldpc_qspa_decode_batch(nbldpc_code *code, const float *L_ch, int B, int maxIT, int *DecodeOutput, int *iter_number, int *ok,
                             float *APP, float *c2v, void *stream);
int nbldpc_qspa_decode_host(int N, int M, int q, int dvmax, int dcmax, const int *vn_weight, const int *vn_linkCNs, const int *vn_linkCNs_GF,
                            const int *cn_weight, const int *cn_linkVNs, const int *cn_linkVNs_GF, const unsigned *TableMultiply,
                            const float *L_ch, int B, int maxIT, int *DecodeOutput, int *iter_number, int *ok, float *APP, float *c2v);
int nbldpc_qspa_exp_host(const float *x, int n, float *y);

/* ---- FHT sum-product, layered schedule ------------------------------------------------------------------------------------------
 *
 * The decoder above with a serial (row by row) schedule; ours as well.  The host statement nbldpc_qspa_layered_decode_host
 * (csrc/nbldpc_qspa_host.hpp, layered = true) is the definition, and the kernel equals it bit for bit.  Everything is as
 * "FHT sum-product" has it -- input and probability vectors, norm and the channel vector, the check-node rule, the iteration loop
 * (APP and decision from p and ALL current c2v, the syndrome, the stop rule, what iter_number, ok and DecodeOutput hold), the
 * outputs APP and c2v, the expressions of csrc/nbldpc_qspa_math.hpp and no other, never contracted -- except the part of an
 * iteration after the syndrome check, which reads:
 *     for rows r = 0 ... M-1 in that order: for every slot t of the row, with variable i and that edge's index d at the variable,
 *     v2c_t = p_i, then for d' ascending, d' != d: v2c_t = norm(v2c_t * c2v_d'), with the c2v AS THEY STAND AT THAT MOMENT (rows
 *     before r already hold this iteration's messages).  Then the check-node rule on the row, and its c2v are stored before row
 *     r + 1 begins.
 * The extrinsic vector is re-formed from p and the other edges' messages; it is never app / c2v (the 2^-40 floors make that
 * quotient inexact), so there is no APP array between rows and the state is that of the flooding decoder.
 * Refusals.  Those of the flooding pair, with the same LDS bound for nbldpc_qspa_layered_decode_batch
 *         4 (N q + M dcmax q) + 4 (N + 4) + q^2  <=  159 * 1024 bytes
 *     (the level tables are read from global memory), and one more, in both calls: a row that lists one variable in two slots is
 *     NBLDPC_EUNSUPPORTED.  nbldpc_code_create accepts such a row when the two slots carry one coefficient (its cross indices take
 *     the first match), and "the other edges of the variable" is not defined for it.  Nothing is launched on a refusal.
 * nbldpc_qspa_layered_decode_batch: all pointers DEVICE memory, asynchronous on `stream`; one workgroup per frame
 *     (k_nb_qspa_layered in nbldpc_last_kernel).  The kernel runs the rows of one dependency level at a time (a row's level is 1 +
 *     the highest level among the earlier rows that share a variable with it: every earlier row that shares a variable has run, no
 *     later one has, and the rows of a level share none), which is the serial order's result bit for bit.  Threads per workgroup:
 *     256 where its waves hold the code's widest level in one pass (4 * max(64 / q, 1) rows), else 512; fixed at
 *     nbldpc_code_create, where the environment variable NBLDPC_QSPA_LAYERED_THREADS = 256 | 512 | 1024 pins it (an experiment
 *     switch; 1024 is never the rule's choice).  The results do not depend on it.  nbldpc_qspa_layered_threads reports it (0 for a
 *     null code).
 * nbldpc_qspa_layered_decode_host: HOST pointers, the argument list of nbldpc_qspa_decode_host, serial. ---- */
int nbldpc_qspa_layered_decode_batch(nbldpc_code *code, const float *L_ch, int B, int maxIT, int *DecodeOutput, int *iter_number,
                                     int *ok, float *APP, float *c2v, void *stream);
int nbldpc_qspa_layered_decode_host(int N, int M, int q, int dvmax, int dcmax, const int *vn_weight, const int *vn_linkCNs,
                                    const int *vn_linkCNs_GF, const int *cn_weight, const int *cn_linkVNs, const int *cn_linkVNs_GF,
                                    const unsigned *TableMultiply, const float *L_ch, int B, int maxIT, int *DecodeOutput,
                                    int *iter_number, int *ok, float *APP, float *c2v);
int nbldpc_qspa_layered_threads(const nbldpc_code *code);

/* ---- FHT sum-product, workspace tier --------------------------------------------------------------------------------------------
 *
 * Both schedules for the codes whose frame state exceeds the LDS bound above (Tanner_74_9_Z128_GF16.txt: 2.1 MB per frame;
 * LDPC_N576_K480_GF256_exp.txt: 285 KB).  The results are those of the host statements nbldpc_qspa_decode_host (layered = 0) /
 * nbldpc_qspa_layered_decode_host (layered != 0) bit for bit -- DecodeOutput, iter_number, ok, APP and c2v -- by the expressions of
 * csrc/nbldpc_qspa_math.hpp and no other, never contracted.  Arguments and return codes are those of nbldpc_qspa_decode_batch.
 * The frame's vectors live in a global-memory workspace slot, p [N][q] floats then the messages [M][dcmax][q] floats, that belongs to
 * one workgroup for the whole launch; the workgroups are persistent and take their frames from a counter.  LDS holds the decisions,
 * 4 flag words, TableMultiply as bytes and NV row slabs of dcmax * q floats, NV = threads / 64 * max(64 / q, 1):
 *         4 (N + 4) + q^2 + 4 NV dcmax q  <=  159 * 1024 bytes.
 * Plan.  threads = the largest of 1024, 512, 256, 128, 64 that meets the bound; layered: the smallest of those that meet it whose NV
 *     holds the code's widest dependency level in one pass, if there is one.  The workspace is allocated and freed stream-ordered by
 *     the call: min(B, 1024, what fits in 2 GiB) slots.
 * Refusals (nothing launched, outputs untouched, nbldpc_last_kernel unchanged).  Those of nbldpc_qspa_decode_batch without its LDS
 *     bound, layered: a row that lists one variable in two slots; and NBLDPC_EUNSUPPORTED where even 64 threads miss the bound above
 *     (q = 256 with dcmax = 96, whatever N) or one slot does not fit in 2 GiB.  A code that fits the LDS tier is accepted as any other.
 * nbldpc_last_kernel reads "k_nb_qspa_ws" / "k_nb_qspa_ws_layered".
 * nbldpc_qspa_ws_plan_host: the plan without a device; info = {threads, LDS bytes, slot bytes, NV}.  widest_level is read for
 *     layered != 0 only.  nbldpc_qspa_ws_info: the same for a code object, with the code's switches applied.  nbldpc_qspa_ws_slots: the
 *     workspace slots (= workgroups) a call with B frames on this code allocates, or a negative return code.
 * Experiment switches, read once at nbldpc_code_create; the results never depend on them: NBLDPC_QSPA_WS_SLOTS = n caps the slots;
 *     NBLDPC_QSPA_WS_THREADS = 64 | 128 | 256 | 512 | 1024 pins the workgroup, and a size that misses the bound is
 *     NBLDPC_EUNSUPPORTED at decode. ---- */
int nbldpc_qspa_ws_decode_batch(nbldpc_code *code, const float *L_ch, int B, int layered, int maxIT, int *DecodeOutput, int *iter_number,
                                int *ok, float *APP, float *c2v, void *stream);
int nbldpc_qspa_ws_plan_host(int N, int M, int q, int dcmax, int widest_level, int layered, int info[4]);
int nbldpc_qspa_ws_info(const nbldpc_code *code, int layered, int info[4]);
int nbldpc_qspa_ws_slots(const nbldpc_code *code, int layered, int B);

const char *nbldpc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
