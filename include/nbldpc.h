/* include/nbldpc.h -- C ABI of the MI355X non-binary LDPC decode path (libnbldpc_hip.so).
 *
 * Drop-in boundary for the reference's message-passing hot path:
 *
 *   reference interface (YongonY/NBLDPC)                      replaced by
 *   --------------------------------------------------------  -----------------------------------------
 *   bool CNBLDPC::Initial(CSimulation&)   NBLDPC.h:42,         nbl_create()  (graph + GF tables + decoder
 *        NBLDPC.cpp:140-377 (graph parse, cross indices,                      parameters; device buffers)
 *        per-algorithm scratch)
 *   int  CNBLDPC::Decoding(double** L_ch, int* DecodeOutput,   nbl_decode_batch()         host buffers
 *        int*, int*)        NBLDPC.h:71, NBLDPC.cpp:607-641    nbl_decode_batch_device()  HBM-resident
 *        -> Decoding_BP :643, Decoding_EMS :778,
 *           Decoding_TEMS :929, Decoding_BS_TEMS :1145               nbl_create_ex() (method 7)
 *   public members L_post / L_v2c / L_c2v  NBLDPC.h:65-68      nbl_read_state()  (parity tests only)
 *   ~CNBLDPC                                                   nbl_destroy()
 *
 * One reference call decodes ONE codeword on the calling thread; one call here decodes a BATCH of B
 * independent codewords (the reference's `parallel` lanes, main.cpp:46) on one GPU.
 * Plain C types only: no exceptions, no exit(); every failure is a negative nbl_status and a message
 * retrievable with nbl_last_error().  There is NO CPU fallback: without a HIP device nbl_create fails.
 */
#ifndef NBLDPC_H
#define NBLDPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBL_ABI_VERSION 1

/* decode methods: the reference's numbering, Simulation.h:3-9 */
#define NBL_METHOD_BP   1 /* exact log-domain QSPA, forward/backward */
#define NBL_METHOD_EMS  2 /* configuration-set EMS, nm/nc truncated   */
#define NBL_METHOD_TEMS 4 /* trellis EMS                              */
#define NBL_METHOD_OSD  6 /* ordered-statistics decoding alone, no iterations: through nbl_create_osd */
#define NBL_METHOD_BS_TEMS 7 /* basic-set trellis EMS: parameters through nbl_create_ex */

typedef enum nbl_status {
	NBL_OK = 0,
	NBL_ERR_ARG = -1,        /* bad argument / inconsistent graph (reference: undefined behaviour or exit(-1)) */
	NBL_ERR_UNSUPPORTED = -2,/* method 3 outside nbl_create_minmax and method 5, which stays unbuilt (reference prints "not developed"
	                            and exits, NBLDPC.cpp:618-638), method 6 without
	                            nbl_create_osd's parameters, method 7 without nbl_create_ex's, a shape the kernels do not serve,
	                            an OSD matrix that is too large or not of full row rank                                        */
	NBL_ERR_NO_DEVICE = -3,  /* no HIP device: there is deliberately no CPU path                               */
	NBL_ERR_HIP = -4,        /* a HIP runtime call failed                                                      */
	NBL_ERR_NOMEM = -5
} nbl_status;

/* Tanner graph exactly as the reference's code file lists it (NBLDPC.cpp:147-205), 0-based indices.
 * Both directions are given because their ORDER is semantically relevant: the order of a check's edges
 * fixes the floating-point association order and the tie-breaks of every check-node algorithm. */
typedef struct nbl_code_desc {
	int32_t N, M, q;            /* CodeLen, ChkLen, GFq                                        */
	const int32_t *var_deg;     /* [N]  VarDegree                                              */
	const int32_t *chk_deg;     /* [M]  ChkDegree                                              */
	const int32_t *var_chk;     /* [E]  VarLink, variable-major                                */
	const int32_t *var_h;       /* [E]  VarLinkGFe                                             */
	const int32_t *chk_var;     /* [E]  ChkLink, check-major                                   */
	const int32_t *chk_h;       /* [E]  ChkLinkGFe                                             */
} nbl_code_desc;

/* Decoder parameters: the fields CNBLDPC::Initial copies out of CSimulation (NBLDPC.cpp:142-143, 267-304). */
typedef struct nbl_params {
	int32_t method;             /* NBL_METHOD_*                                                */
	int32_t max_iter;           /* sim.maxIter                                                 */
	int32_t ems_nm, ems_nc;     /* sim.ems_nm, sim.ems_nc                                      */
	double  ems_factor, ems_offset;
	int32_t tems_nr, tems_nc;   /* sim.tems_nr, sim.tems_nc                                    */
	double  tems_factor, tems_offset;
	int32_t fixed_iters;        /* 0: a codeword stops at its first zero syndrome (reference).   */
	                            /* 1: every codeword runs max_iter iterations (throughput runs); */
	                            /*    outputs are frozen at the first zero syndrome either way.  */
	int32_t poll_every;         /* fixed_iters==0: ask the device every k iterations whether all */
	                            /* codewords are done (0 = never, run max_iter launches)         */
	int32_t max_batch;          /* workspace is sized for this many codewords (grows on demand)  */
} nbl_params;

typedef struct nbl_decoder nbl_decoder;

/* gf_mul: q*q multiplication table, gf_inv: q inverses (gf_inv[0] ignored) -- the tables CGF::Initial loads
 * from ./SRC/Arith.Table.GF.<q>.txt (GF.cpp:81-113).  Addition is XOR: the table must be that of GF(2)[x] / m(x) in the
 * polynomial basis for an irreducible m of degree p (q = 2^p), any of them -- m need not be primitive, nor the one the reference
 * ships for this q.  The irreducible polynomial is recovered from the table (q | gf_mul[2][q/2]) and the tables are checked in
 * full at creation, before anything is indexed by one of their entries and before the device is touched: every gf_mul entry
 * below q, row and column 0 zero, every gf_mul[a][b] the shift-and-XOR product modulo m, and for every a in 1 .. q-1
 * gf_inv[a] < q with gf_mul[a][gf_inv[a]] == 1 (which no reducible m can meet).  Anything else is NBL_ERR_ARG, the message
 * names the first offending entry.
 * Shapes: q = 4 .. 256 (a power of two), check and variable degrees up to 8, ems_nm <= q, T-EMS with p * (largest check
 * degree) <= 32 (q = 2^p; the path code of TEMS_ConstructConf in 32 bits; nbl_create_tems_wide has neither limit); anything else is NBL_ERR_UNSUPPORTED / NBL_ERR_ARG
 * with a message, at creation, never at the first decode. */
nbl_status nbl_create(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv,
                      const nbl_params *params, int device, nbl_decoder **out);

/* Parameters of the methods nbl_params does not carry: basic-set T-EMS (NBL_METHOD_BS_TEMS), the fields CNBLDPC::Initial copies
 * for method 7 (NBLDPC.cpp:332-337; profile lines "BSTEMS Nm / Nc / Factor / Offset").
 *   bs_nm      elements of the basic set, 1 <= bs_nm <= q - 1 (NBL_ERR_ARG otherwise: the reference reads past its arrays), and
 *              at most 16 (NBL_ERR_UNSUPPORTED above: the kernel enumerates the configurations as masks of bs_nm bits)
 *   bs_nc      largest number of deviating columns of a configuration, >= 0
 *   bs_factor  c2v scaling (divisor, != 0), bs_offset its dead zone, as ems_/tems_factor and _offset */
typedef struct nbl_params_ext {
	int32_t bs_nm, bs_nc;
	double  bs_factor, bs_offset;
} nbl_params_ext;
/* nbl_create with the extension parameters; ext may be NULL (then it IS nbl_create, and method 7 is NBL_ERR_UNSUPPORTED).
 * ext is read for method 7 only. */
nbl_status nbl_create_ex(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv,
                         const nbl_params *params, const nbl_params_ext *ext, int device, nbl_decoder **out);

/* Ordered-statistics decoding (OSD.h): post-processing of the frames an iterative method leaves unconverged (order >= 0, methods
 * 1/2/4/7, NBLDPC.cpp:769-775 and its twins), or the whole decode (NBL_METHOD_OSD: Decoding_OSD_bit(L_ch, .., flag = 1), order 0
 * when order < 0, flag taken as 1, converged = 0 and iters = 0 on return).  Post-processing changes only out_sym of the codewords
 * that did not converge; converged, iters and the message state stay as the iterations left them (the reference, too, returns
 * "not converged" after OSD).  With max_iter = 0 the reference never runs the post-processing, and neither does this.
 *   order     sim.OSD_order: -1 = off (methods 1/2/4/7); 0 .. 3; above 3 behaves as 3 (OSD.h:139-165 are ">=" tests)
 *   flag      sim.OSD_flag: 1 = reliabilities and base word from L_ch; 0 = from the factor-weighted sum of the posteriors of every
 *             iteration (NBLDPC.cpp:687) and the last iteration's decisions
 *   factor    sim.OSD_factor (alpha), read by flag 0 only
 *   crc_len   sim.crcLen; crc_rows sim.crc_correctLen: CRC rows put above the binary parity-check matrix (OSD.h:37-48, 472-509);
 *             crc_rows > 0 needs crc_len 8, 16 or 24 (NBL_ERR_ARG otherwise: the reference's generator is empty and its
 *             elimination never ends)
 *   gf_mat    [q][p][p] bytes, gf_mat[e][l][k] = GFElement[e].ValueMatric[l][k]: the binary image of "multiply by e" as the caller's
 *             loader left it.  The reference's loader (GF.cpp:137) reads q-2 of the q-1 matrices, so alpha^(q-2)'s stays zero; pass
 *             the same to reproduce it, or the full set for the true binary image.  The matrix of element 1 must be the identity
 *             (NBL_ERR_ARG otherwise); the layout lists powers of x, so a loader fills it for a primitive modulus only.
 * The binary matrix [crc_rows; H_bit] ((crc_rows + M p) rows of N p bits, q = 2^p) is built and checked once, at creation, before
 * any device call: N p above NBL_OSD_MAX_BITS (the matrix and the candidate codewords live in one workgroup's LDS; every shipped
 * code fits) and a matrix without full row rank (the reference's elimination never ends on one) are NBL_ERR_UNSUPPORTED.
 * Known deviation: positions of equal reliability are ordered by index (the reference's std::sort is not stable); this only
 * matters for exact ties, e.g. the all-zero LLRs of punctured symbols under flag 1.
 * osd == NULL: this is nbl_create_ex (and method 6 is NBL_ERR_UNSUPPORTED). */
#define NBL_OSD_MAX_BITS 1024
typedef struct nbl_osd_params {
	int32_t order;
	int32_t flag;
	double  factor;
	int32_t crc_len;
	int32_t crc_rows;
	const uint8_t *gf_mat;
} nbl_osd_params;
nbl_status nbl_create_osd(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                          const nbl_params_ext *ext, const nbl_osd_params *osd, int device, nbl_decoder **out);
void nbl_destroy(nbl_decoder *dec);

/* ---- the layered (check-serial) schedule for EMS ------------------------------------------------------------------------------
 * Every other entry point runs the reference's flooding schedule: in each iteration all variables update, then all checks
 * (NBLDPC.cpp:805-918).  In a layered schedule a check reads the messages its neighbours wrote earlier in the SAME iteration, and a
 * frame converges in fewer iterations.  Nothing in the reference computes it; the operation is defined here, operation by operation,
 * so that independent implementations agree (tests/layered_ref.py restates it in numpy on top of the reference-pinned check-node
 * update).
 *   A layer assignment layer_of[M] maps every check to a layer 0 .. n_layers-1; every layer is non-empty and no two checks of one
 *   layer share a variable.  The result depends on the assignment, so the assignment is an input.
 *   State: c2v[E], all zero before iteration 1.  Iteration it = 1 .. max_iter:
 *   1. Tentative decision and syndrome, exactly as flooding (NBLDPC.cpp:808-846): post[n] = L_ch[n], then += c2v of the variable's
 *      edges in the variable's edge order; DecideLLRVector; the syndrome.  The first zero syndrome freezes out_sym, sets converged
 *      and iters = it (and, with fixed_iters == 0, ends the frame: its c2v stay as iteration it-1 left them).  fixed_iters and
 *      poll_every keep their meaning.
 *   2. For l = 0 .. n_layers-1, for every check m with layer_of[m] == l:
 *        for every edge k of m, with variable n:
 *          P = L_ch[n];  P += c2v[e] for each edge e of n, in n's edge order, reading the CURRENT values;  v2c_k = P - c2v[(m,k)]
 *          (the reference's AddLLRVector / MinusLLRVector expressions, :810-817 and :855; slot 0 of a vector is 0; no other
 *          normalisation)
 *        c2v[(m, .)] = the EMS check-node update of v2c_0 .. v2c_{dc-1} (:859-917): the canonical, residue-free value every EMS
 *        kernel of this library computes.
 *      The order inside a layer is immaterial: the checks of a layer share no variable.
 *   With one layer per check, in check order, this is the serial-C schedule.
 * nbl_layer_greedy: pure host arithmetic, no device: the library's default assignment.  Checks in ascending index, each gets the
 * smallest layer that holds no check sharing a variable with it.  Returns n_layers, or a negative nbl_status.
 * nbl_create_layered: nbl_create with this schedule; layer_of == NULL: nbl_layer_greedy's.  NBL_METHOD_EMS only (no OSD, no
 * extension parameters).  Refused at creation, before the device is touched, with a message: NBL_ERR_ARG for a layer index below 0,
 * an empty layer below the largest index used, two checks of one layer sharing a variable (the message names both checks and the
 * variable); NBL_ERR_UNSUPPORTED for any other method (methods 1, 4 and 7 damp their variable-to-check messages against the
 * previous iteration's; T-EMS has its layered schedule behind nbl_create_layered_ex below, log-QSPA behind nbl_create_layered_bp, method
 * 7 stays flooding-only); and
 * everything nbl_create refuses, the same way.
 * Every decode call, the demodulator, channel, transmitter and error count work unchanged on such a decoder.  nbl_read_state returns
 * post (with nbl_set_record_state) and c2v as defined above; EMS never materialises v2c: a non-NULL v2c is NBL_ERR_UNSUPPORTED.
 * nbl_get_layers: the assignment in use (host arrays; either may be NULL); NBL_ERR_ARG on a flooding decoder. */
int32_t nbl_layer_greedy(const nbl_code_desc *code, int32_t *layer_of /* [M] */);
nbl_status nbl_create_layered(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv,
                              const nbl_params *params, const int32_t *layer_of, int device, nbl_decoder **out);
nbl_status nbl_get_layers(const nbl_decoder *dec, int32_t *layer_of, int32_t *n_layers);

/* ---- the layered schedule for T-EMS, with its per-edge damping ------------------------------------------------------------------
 * The reference's T-EMS damps every variable-to-check vector against the SAME EDGE's vector of the previous iteration
 * (NBLDPC.cpp:1029-1052): where their hard decisions differ, the new vector becomes 0.25 old + 0.75 new.  An edge belongs to exactly
 * one check, so a check visited in its layer can do this itself, and the layered schedule above carries over.  Defined here operation
 * by operation (tests/layered_tems_ref.py restates it in numpy on top of the reference-pinned T-EMS check-node update; DESIGN.md
 * section 5g):
 *   Layer assignment: as above -- the same validity rules, the same nbl_layer_greedy.
 *   State: c2v[E], all zero before iteration 1; v2c[E], with v2c[(m,k)] = L_ch[n] for the edge's variable n before iteration 1
 *   (:934-940).  Vectors have q slots; slot 0 is 0.  Iteration it = 1 .. max_iter:
 *   1. Tentative decision and syndrome exactly as flooding and as layered EMS (:977-1015).  The first zero syndrome freezes out_sym,
 *      sets converged and iters = it (and, with fixed_iters == 0, ends the frame: its c2v AND v2c stay as iteration it-1 left them).
 *   2. For l = 0 .. n_layers-1, for every check m with layer_of[m] == l:
 *        for every edge k of m, with variable n:
 *          P = L_ch[n];  P += c2v[e] for each edge e of n, in n's edge order, reading the CURRENT values;  raw = P - c2v[(m,k)]
 *          old = v2c[(m,k)]
 *          in_k = raw, unless DecideLLRVector(raw) != DecideLLRVector(old): then in_k[a] = 0.25 * old[a] + 0.75 * raw[a], each product
 *          rounded, then the sum rounded, no contraction (:1046)
 *          v2c[(m,k)] = in_k
 *        c2v[(m, .)] = the T-EMS check-node update of in_0 .. in_{dc-1} (:1055-1129): the canonical, residue-free value every T-EMS
 *        kernel of this library computes.
 *   fixed_iters, poll_every, the active list and the device-buffer entry points keep their meaning.
 * nbl_create_layered_ex: flags == 0 IS nbl_create_layered (the same refusals, the same texts).  NBL_LAYERED_DAMPED with NBL_METHOD_TEMS
 * runs the schedule above; with NBL_METHOD_EMS the flag is inert (EMS has no damping: the decoder is nbl_create_layered's); any other
 * method is NBL_ERR_UNSUPPORTED (log-QSPA has its own entry point, nbl_create_layered_bp below, with its own parity statement; BS-TEMS
 * has no single-check oracle entry point, so its schedule could not be pinned); an unknown flag bit is NBL_ERR_ARG.  Everything nbl_create refuses is
 * refused the same way (T-EMS with log2(q) * maxdc > 32 included), and a shape whose check needs more than 160 KB of LDS is refused
 * here, not at the first decode; all of it before the device is touched.  On a damped T-EMS decoder nbl_read_state returns v2c as
 * defined above (variable-major edge order, like c2v) instead of refusing it; nbl_get_layers works. */
#define NBL_LAYERED_DAMPED 1
nbl_status nbl_create_layered_ex(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv,
                                 const nbl_params *params, const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out);

/* ---- the layered schedule for log-QSPA, with its per-edge damping ---------------------------------------------------------------
 * The reference's log-QSPA damps like its T-EMS, per edge against the SAME EDGE's vector of the previous iteration (NBLDPC.cpp:730-741),
 * with the blend 0.5 old + 0.5 new where the hard decisions differ; so a check visited in its layer can do it itself here too.
 * Defined operation by operation (tests/layered_bp_ref.py restates it in numpy on top of the oracle's log-QSPA check-node update;
 * DESIGN.md section 5j):
 *   Layer assignment: as above -- the same validity rules, the same refusal texts, the same nbl_layer_greedy for layer_of == NULL.
 *   State: c2v[E], all zero before iteration 1; v2c[E], with v2c[(m,k)] = L_ch[n] for the edge's variable n before iteration 1
 *   (:647-655).  Vectors have q slots; slot 0 is 0.  Iteration it = 1 .. max_iter:
 *   1. Tentative decision and syndrome exactly as flooding (:676-709).  The first zero syndrome freezes out_sym, sets converged and
 *      iters = it (and, with fixed_iters == 0, ends the frame: its c2v AND v2c stay as iteration it-1 left them).
 *   2. For l = 0 .. n_layers-1, for every check m with layer_of[m] == l:
 *        for every edge k of m, with variable n:
 *          P = L_ch[n];  P += c2v[e] for each edge e of n, in n's edge order, reading the CURRENT values;  raw = P - c2v[(m,k)]
 *          old = v2c[(m,k)]
 *          in_k = raw, unless DecideLLRVector(raw) != DecideLLRVector(old): then in_k[a] = 0.5 * old[a] + 0.5 * raw[a], each product
 *          rounded, then the sum rounded, no contraction (:739)
 *          v2c[(m,k)] = in_k
 *        c2v[(m, .)] = the log-QSPA check-node update of in_0 .. in_{dc-1} (:747-767), as every log-QSPA kernel of this library
 *        evaluates it (FP64 log-sum-exp; the reference's is 80-bit and sequential).
 *   Parity is the method's own, as for flooding log-QSPA: hard decisions, converged flags and iteration counts equal those of the
 *   FP64 restatement, post / c2v / v2c agree with it within 1e-9 of the largest magnitude; not bit for bit.
 *   fixed_iters, poll_every, the active list and the device-buffer entry points keep their meaning; so do bit-LLR input, soft output
 *   (plain and extrinsic), the demodulators, channel, transmitter, error count and the iterative-demapping loop.
 * nbl_create_layered_bp: nbl_create with this schedule.  NBL_METHOD_BP only (no OSD, no extension parameters); there are no flags.
 * Refused at creation, before the device is touched, with a message: NBL_ERR_UNSUPPORTED for any method but 1 (the message names
 * method 1 and points to nbl_create_layered and nbl_create_layered_ex); every assignment error of nbl_create_layered, with its status
 * and text; everything nbl_create refuses, the same way.  No shape is refused for its LDS: a check takes (3 maxdc + 5) q 8 bytes,
 * 59,392 B at q = 256 and degree 8.  nbl_read_state returns post (with nbl_set_record_state), c2v and v2c as defined above, both in
 * variable-major edge order; nbl_get_layers works. */
nbl_status nbl_create_layered_bp(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv,
                                 const nbl_params *params, const int32_t *layer_of, int device, nbl_decoder **out);

/* ---- FHT sum-product decoding: the fast check node of non-binary BP, flooding and layered ----------------------------------------
 * Over GF(2^p) the box-plus of the sum-product rule is an XOR convolution of probability vectors, and the Walsh-Hadamard transform
 * (WHT) turns it into a pointwise product: a check costs 2 dc transforms of q log2 q butterflies instead of 3 (dc - 2) sums of q^2
 * terms.  The transform subtracts, so outputs far below a vector's largest are rounding noise and are floored.  This is therefore NOT
 * another evaluation of method 1's check node: it is a decoder kind of its own, with its own definition and its own parity statement
 * (tests/fht_ref.py restates it in numpy).
 *   The FHT check-node update of inputs in_0 .. in_{dc-1} (q-vectors of LLRs, slot 0 = 0) with edge coefficients h_d.  All arithmetic is
 *   IEEE double, every product and every sum rounded on its own, no contraction:
 *   1. Check domain: p_d[h_d a] = in_d[a] (as the log-QSPA check node does, NBLDPC.cpp:1623-1632).
 *   2. m_d = max_y p_d[y];  u_d[y] = exp(p_d[y] - m_d).
 *   3. U_d = WHT(u_d), in place: stages with stride s = 1, 2, 4, .., q/2 in that order; in a stage, for every i with bit s clear,
 *      (x[i], x[i+s]) <- (x[i] + x[i+s], x[i] - x[i+s]).  The order inside a stage is immaterial.
 *   4. Fwd_1 = U_0, Fwd_{k+1} = Fwd_k * U_k;  Bwd_{dc-2} = U_{dc-1}, Bwd_{k-1} = Bwd_k * U_k (elementwise);
 *      V_0 = Bwd_0, V_{dc-1} = Fwd_{dc-1}, otherwise V_d = Fwd_d * Bwd_d.  (dc = 2: V_0 = U_1, V_1 = U_0.)
 *   5. v_d = WHT(V_d), the same stages, left unnormalised (the factor 1/q cancels in step 7).
 *   6. t = max_y v_d[y] (> 0: sum_y v_d[y] = q * prod_k U_k[0] > 0);  v'_d[y] = max(v_d[y], t * 2^-NBL_FHT_FLOOR_LOG2).  The floor is part
 *      of the method, not a tuning knob: no c2v entry lies more than 40 ln 2 = 27.7 nats below its vector's largest; an entry at the
 *      floor carries a relative error of about 2^-10, anything above it proportionally less.
 *   7. c_d[y] = log(v'_d[y]) - log(v'_d[0]), c_d[0] = 0;  c2v_d[a] = c_d[h_d a].
 *   Consequences: given equal u the v are bit-identical between implementations (steps 3-5 are adds, subtracts and products in a fixed
 *   order); only exp and log differ.  Inputs are assumed finite.  A vector wider than about 745 nats becomes one-hot and its partners'
 *   outputs saturate at the floor: unlike log-QSPA the method has a bounded range by construction.
 *   Schedules.  Flooding (flags 0): the reference's log-QSPA iteration (NBLDPC.cpp:643-775) -- decision, syndrome, variable-node pass
 *   with the 0.5 / 0.5 per-edge damping -- with the check-node update above in place of :747-767.  Layered (NBL_FHT_LAYERED): word for
 *   word the schedule of nbl_create_layered_bp above with the same replacement: the same layer rules, the same nbl_layer_greedy, the
 *   same v2c state and damping.
 *   Parity.  For a vector x let w(x) = exp(x - max x), the implicit 0 of slot 0 included.  Hard decisions, converged flags and
 *   iteration counts equal those of the FP64 numpy restatement on inputs whose decisions have a margin; for post, c2v and v2c,
 *   |w(x_gpu) - w(x_ref)| stays within 16 times the deviation between the restatement in FP64 and in 80-bit arithmetic
 *   (tests/fht_ref.py records it per case).  A statement in the probability domain: LLRs of entries near the floor are not pinned.
 * nbl_create_fht: NBL_METHOD_BP only (no OSD, no extension parameters).  flags 0 = flooding (a non-NULL layer_of is NBL_ERR_ARG);
 * NBL_FHT_LAYERED = layered, layer_of == NULL selects the greedy assignment; an unknown flag bit is NBL_ERR_ARG.  Any other method is
 * NBL_ERR_UNSUPPORTED (the message names method 1); every assignment error of nbl_create_layered keeps its status and text; everything
 * nbl_create refuses is refused the same way, except the check-degree limit, which is 32 here (NBL_FHT_MAX_CHECK_DEGREE: check degrees
 * 2 .. 32, variable degrees 1 .. 8; a larger check is NBL_ERR_ARG and the message names 32); all of it before the device is touched.  The
 * update above is generic in dc: a code whose checks all have degree 8 or less runs it with the transformed inputs in registers, any other
 * code in a layout whose storage does not grow with the degree; the two evaluate the same operations in the same order and give the same
 * bits.  No shape is refused for its LDS (maxdc q 8 bytes, at most 64 KB, at q = 256 and degree 32).  Every decode entry point (host, device, bits, samples, prior, csi, idd, resident), soft output (plain and
 * extrinsic), fixed_iters, poll_every and the active list, the transmitter, channel and error count work unchanged on such a decoder.
 * nbl_read_state returns post, c2v and v2c as on the corresponding log-QSPA decoder; nbl_get_layers works on the layered kind and is
 * NBL_ERR_ARG on the flooding kind.  Method 1 through nbl_create stays the exact log-QSPA. */
#define NBL_FHT_FLOOR_LOG2 40
#define NBL_FHT_LAYERED 1u
#define NBL_FHT_MAX_CHECK_DEGREE 32
nbl_status nbl_create_fht(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                          const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out);

/* ---- Single-precision FHT sum-product decoding: FP32 messages, flooding and layered ------------------------------------------------
 * The FHT decoder above has no reference to match -- it is defined here, operation by operation -- so it is the one decoder kind whose
 * precision can change without touching a parity statement made against the reference.  nbl_create_fht32 is word for word the FHT decoder
 * of nbl_create_fht, flooding (flags 0) or layered (NBL_FHT32_LAYERED), with these replacements (tests/fht32_ref.py restates it in
 * numpy: fht_ref.decode_flooding / decode_layered with dtype = np.float32):
 *   1. Channel vectors.  Lf[n][a] = (float) L_ch[n][a], round to nearest even, once per decode call.  Every front end (host or device
 *      LLRs, bit LLRs, the demodulators, priors, gains, the channel) produces the FP64 L_ch it produces on every other decoder; one
 *      narrowing launch follows it.  Inputs are assumed finite and inside the binary32 range.
 *   2. Arithmetic.  Everything the iterations compute is IEEE binary32, every product and every sum rounded on its own, no contraction:
 *      the a-posteriori sum in the variable's edge order starting from Lf, DecideLLRVector on the float vector (the same tie rule),
 *      raw = P - c2v, the 0.5 / 0.5 per-edge damping where decisions differ, the initial v2c = Lf, and steps 1-7 of the check-node update.
 *   3. The floor (step 6) is t * 2^-NBL_FHT32_FLOOR_LOG2 = t * 2^-16: no c2v entry lies more than 16 ln 2 = 11.09 nats below its vector's
 *      largest.  The transform's rounding noise must stay well below the floor, as it does in FP64 (2^-40 against 2^-53): the largest
 *      |v32 - v80| / t measured on the CPU is 2^-20.7 (q = 256, degree 8), so an entry at the floor carries a relative error of about 2^-5
 *      (0.03 nats) where the FP64 kind's figure is 2^-10.
 *   4. exp and log: any evaluation within 2 ulp of binary32 (the device library's expf / logf qualify; a bare hardware exp2 on
 *      x * log2(e) does not for |x| above about 8, where the product's rounding alone is |x| 2^-24 relative).
 *   5. Limits.  Check degrees 2 .. 8, variable degrees 1 .. 8: |U[y]| <= q, so a product of up to 7 transformed vectors stays below 2^56
 *      and its transform below 2^64; at degree 32 it would leave binary32's range.  A larger check is NBL_ERR_ARG (the message names
 *      nbl_create_fht32, the degree found and 8, and points to nbl_create_fht; nbl_create_fht32_wide, below, takes such a code in single
 *      precision).  Any method but 1 is NBL_ERR_UNSUPPORTED (the message names
 *      method 1); an unknown flag bit is NBL_ERR_ARG; a non-NULL layer_of with flags 0 is NBL_ERR_ARG; every assignment error of
 *      nbl_create_layered keeps its status and text; everything else nbl_create refuses is refused the same way.  No OSD, no extension
 *      parameters.  All of it before the device is touched.
 *   6. State and soft output.  nbl_read_state returns post (with nbl_set_record_state), c2v and v2c as doubles that are the EXACT widening
 *      of the float state; order and early-exit rules are the FHT kind's.  nbl_soft_output* keeps its definition unchanged: P = L_ch (the
 *      caller's FP64 vector, not Lf) plus the c2v exactly as nbl_read_state returns them, summed in double -- bit for bit the sum above
 *      over this decoder's own read_state.  The iterative-demapping loop, a chain of public calls, needs nothing new.
 *   7. Every decode entry point (host, device, bits, samples, prior, csi, idd, resident, noise), fixed_iters, poll_every and the active
 *      list, the transmitter, channel, fading and error count work unchanged on such a decoder; nbl_get_layers works on the layered kind
 *      and is NBL_ERR_ARG on the flooding kind.  The FP64 copies of c2v / v2c / post exist from the first call that reads the state
 *      (nbl_read_state, nbl_soft_output*, a demapping loop of several passes) and count in nbl_workspace_bytes from then on.
 *   8. Parity, the method's own.  Hard decisions, converged flags and iteration counts equal those of the float32 numpy restatement on
 *      inputs whose decisions have a margin; for post, c2v and v2c, |w(x_gpu) - w(x_ref)| stays within 16 x D32, the case's recorded
 *      deviation between two evaluations of the restatement: numpy's float32 exp / log, and exp / log taken in float64 and rounded once
 *      to float32 (how far one rounding of exp / log moves the state: the only place implementations may differ).  Nothing is claimed
 *      about closeness to the FP64 kind; DESIGN.md section 5q records what was measured. */
#define NBL_FHT32_FLOOR_LOG2 16
#define NBL_FHT32_LAYERED 1u
nbl_status nbl_create_fht32(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                            const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out);

/* ---- Single-precision FHT decoding for high-rate codes: check degrees up to 32, flooding and layered -----------------------------------
 * nbl_create_fht32_wide: NBL_METHOD_BP only (no OSD, no extension parameters).  nbl_create_fht32 itself does not change: it keeps its
 * limit of 8, its refusal text and its plan.  Everything in the statement above holds here (items 1-8: float channel vectors narrowed
 * once, all arithmetic in binary32 with no contraction, the floor at 2^-16, exp / log within 2 ulp, the exact widening in
 * nbl_read_state, soft output, every decode entry point).  A code whose checks all have degree 8 or less gets exactly the decoder
 * nbl_create_fht32 would make.  A code with a check above degree 8 runs the wide programme, whose check-node update has one more step
 * (tests/fht32_wide_ref.py restates it in numpy):
 *   3a. Let e_d be the integer with 2^e_d <= U_d[0] < 2^(e_d+1).  (U_d[0] = sum_y u_d[y] >= 1, because one u is exactly 1 and none is
 *       negative; U_d[0] <= q.)  U_d <- U_d * 2^(-e_d), every slot: a multiplication by a power of two.  Steps 4-7 run on the scaled
 *       vectors, unchanged.
 *   Range.  Unscaled, |U[y]| <= q: a product of 31 transformed vectors can reach q^31 = 2^248 at GF(256), and a flat input -- the
 *   all-zero channel vector of a punctured symbol -- makes U_d[0] = q exactly, so at degree 32 the overflow is the ordinary case.  Scaled,
 *   |U[y]| < 2, every product stays below 2^31, every transform below 2^39, and t >= V_d[0] >= 1 (the largest of v_d is at least their
 *   mean, V_d[0], a product of values in [1, 2)).
 *   Exactness.  Scaling by a power of two is exact unless a value is subnormal.  Every later operation is a product, a sum, or a maximum
 *   followed by a difference of logs, so the scale cancels in step 7 and the floor of step 6 is relative to the vector's own largest: a
 *   scaled and an unscaled evaluation of one check differ only in how log rounds a scaled argument in step 7.  The two programmes are
 *   therefore NOT bit-identical on a code both run; each carries the parity statement of item 8 against its own restatement (16 x the
 *   case's recorded deviation between the two evaluations of exp / log; tests/fht32_wide_ref.py records D32W per case).
 *   Noise.  The largest |v32 - v80| / t measured on the CPU at degree 32 is 2^-19.56 (q = 256), about 3.5 bits below the floor; the tests
 *   hold every case they run to 2^-18.
 *   flags 0 = flooding (a non-NULL layer_of is NBL_ERR_ARG); NBL_FHT32_WIDE_LAYERED = layered, layer_of == NULL selects the greedy
 *   assignment; an unknown flag bit is NBL_ERR_ARG.  Limits: check degrees 2 .. 32 (NBL_FHT32_MAX_CHECK_DEGREE; a larger check is
 *   NBL_ERR_ARG, the message names this entry point, the degree found and 32); variable degrees stay 1 .. 8, with nbl_create's text.  Any
 *   other method is NBL_ERR_UNSUPPORTED (the message names method 1); every assignment error of nbl_create_layered keeps its status and
 *   text; everything else nbl_create refuses is refused the same way; all of it before the device is touched.  No shape is refused for
 *   its LDS (maxdc q 4 bytes, at most 32 KB, at q = 256 and degree 32).
 *   Every other entry point but nbl_create_fht, nbl_create_ems_wide, nbl_create_tems_wide and nbl_create_bp_wide keeps its check-degree
 *   limit of 8. */
#define NBL_FHT32_MAX_CHECK_DEGREE 32
#define NBL_FHT32_WIDE_LAYERED 1u
nbl_status nbl_create_fht32_wide(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                 const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out);

/* ---- EMS decoding for high-rate codes: check degrees up to 32, flooding and layered ------------------------------------------------
 * nbl_create_ems_wide: NBL_METHOD_EMS only (no OSD, no extension parameters).  There is no new arithmetic: a check's output is the
 * canonical, residue-free EMS value defined above (the maximum over conf(q,1) U conf(nm,nc) of the left-to-right sums over the other
 * edges in index order), which is generic in the check degree; post, c2v, decisions, flags and iteration counts equal the canonical
 * oracle's bit for bit at every degree.
 *   flags 0: word for word the flooding EMS decoder of nbl_create (a non-NULL layer_of is NBL_ERR_ARG).  NBL_EMS_WIDE_LAYERED: word for
 *   word the schedule of nbl_create_layered -- the same layer rules and refusal texts, nbl_layer_greedy for layer_of == NULL.  An unknown
 *   flag bit is NBL_ERR_ARG.
 *   Limits: check degrees 2 .. 32 (NBL_EMS_MAX_CHECK_DEGREE; a larger check is NBL_ERR_ARG, the message names this entry point, the degree
 *   found and 32); variable degrees stay 1 .. 8, with nbl_create's text.  Any other method is NBL_ERR_UNSUPPORTED (the message names
 *   method 2).  A check is run by one workgroup whose LDS holds [maxdc][q] inputs, the lists [maxdc][nm] (12 bytes an entry), three
 *   [layers][q] DP arrays (layers = nc + 1, or 1 when nc >= maxdc - 1) and one [q] vector; a shape that needs more than 160 KB is
 *   NBL_ERR_UNSUPPORTED and the message names the byte count (nm = q = 256 at degree 32 is one).  Everything else nbl_create refuses is
 *   refused the same way; all of it before the device is touched.
 *   A code whose checks all have degree 8 or less gets exactly the decoder nbl_create / nbl_create_layered would make.  Every decode entry
 *   point (host, device, bits, samples, prior, csi, idd, resident), soft output (plain and extrinsic), fixed_iters, poll_every and the
 *   active list, the transmitter, channel and error count work unchanged on such a decoder.  nbl_read_state returns post and c2v as on the
 *   corresponding EMS decoder (a non-NULL v2c is refused on the layered kind, as there); nbl_get_layers works on the layered kind.
 *   Every other entry point but nbl_create_fht, nbl_create_fht32_wide, nbl_create_tems_wide and nbl_create_bp_wide keeps its check-degree limit
 *   of 8. */
#define NBL_EMS_MAX_CHECK_DEGREE 32
#define NBL_EMS_WIDE_LAYERED 1u
nbl_status nbl_create_ems_wide(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                               const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out);

/* ---- T-EMS decoding for high-rate codes: check degrees up to 32 over any field, flooding and layered ----------------------------------
 * nbl_create_tems_wide: NBL_METHOD_TEMS only (no OSD, no extension parameters).  There is no new arithmetic: dW and Eta of a check are
 * the smallest (cost, path in enumeration order) over the paths with at most tems_nc deviations inside the tems_nr marks, costs as
 * left-to-right sums -- the T-EMS check node defined above, which is generic in the check degree; out_sym, converged, iters, post, c2v
 * and v2c equal the canonical oracle's bit for bit at every degree.  What nbl_create cannot hold above log2(q) * (check degree) = 32 is
 * the path of a check sum as base-q digits in one 32-bit word; here a path is stored as its at most NBL_TEMS_WIDE_MAX_NC = 4 deviations
 * (column, symbol) in one 64-bit word that orders like the digit string.
 *   flags 0: word for word the flooding T-EMS decoder of nbl_create (a non-NULL layer_of is NBL_ERR_ARG).  NBL_TEMS_WIDE_LAYERED: word for
 *   word the damped layered schedule of nbl_create_layered_ex(.., NBL_LAYERED_DAMPED) -- the same layer rules and refusal texts,
 *   nbl_layer_greedy for layer_of == NULL.  An unknown flag bit is NBL_ERR_ARG.
 *   Limits: check degrees 2 .. 32 (NBL_TEMS_MAX_CHECK_DEGREE; a larger check is NBL_ERR_ARG, the message names this entry point, the degree
 *   found and 32); variable degrees stay 1 .. 8, with nbl_create's text; nbl_create's limit log2(q) * (largest check degree) <= 32 does not
 *   apply.  Any other method is NBL_ERR_UNSUPPORTED (the message names method 4).  On a code with a check above degree 8 or with
 *   log2(q) * (largest check degree) > 32, tems_nc above 4 is NBL_ERR_UNSUPPORTED (the message names both numbers), and a check is run by
 *   one workgroup whose LDS holds [maxdc][q] dU, the DP states [2][nc + 1][q] of 16 bytes, at most min(nr, maxdc) (q - 1) list entries of
 *   16 bytes and two [q] vectors; a shape that needs more than 160 KB is NBL_ERR_UNSUPPORTED and the message names the byte count.
 *   Everything else nbl_create refuses is refused the same way; all of it before the device is touched.
 *   Any other code gets exactly the decoder nbl_create / nbl_create_layered_ex would make.  Every decode entry point (host, device, bits,
 *   samples, prior, csi, idd, resident), soft output (plain and extrinsic), fixed_iters, poll_every and the active list, the transmitter,
 *   channel and error count work unchanged on such a decoder.  nbl_read_state returns post, c2v and v2c as on the corresponding T-EMS
 *   decoder; nbl_get_layers works on the layered kind.
 *   Every other entry point but nbl_create_fht, nbl_create_fht32_wide, nbl_create_ems_wide and nbl_create_bp_wide keeps its check-degree limit
 *   of 8. */
#define NBL_TEMS_MAX_CHECK_DEGREE 32
#define NBL_TEMS_WIDE_LAYERED 1u
nbl_status nbl_create_tems_wide(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out);

/* ---- Exact log-QSPA for high-rate codes: check degrees up to 32, flooding and layered --------------------------------------------------
 * nbl_create_bp_wide: NBL_METHOD_BP only (no OSD, no extension parameters).  There is no new arithmetic: a check's output is the
 * log-QSPA update (forward and backward partials, XOR convolutions in the log-sum-exp semiring) as every log-QSPA kernel of this library
 * evaluates it, which is generic in the check degree.  Parity is the method's own: hard decisions, converged flags and iteration counts
 * equal those of the FP64 restatement on inputs whose decisions have a margin; post, c2v and v2c agree with it within 1e-9 of the largest
 * magnitude.  (FHT decoding, nbl_create_fht, is a decoder kind of its own with a floor; this is the exact method it is measured against.)
 *   flags 0: word for word the flooding log-QSPA decoder of nbl_create (a non-NULL layer_of is NBL_ERR_ARG).  NBL_BP_WIDE_LAYERED: word for
 *   word the schedule of nbl_create_layered_bp -- the same layer rules and refusal texts, nbl_layer_greedy for layer_of == NULL.  An
 *   unknown flag bit is NBL_ERR_ARG.
 *   Limits: check degrees 2 .. 32 (NBL_BP_MAX_CHECK_DEGREE; a larger check is NBL_ERR_ARG, the message names this entry point, the degree
 *   found and 32); variable degrees stay 1 .. 8, with nbl_create's text.  Any other method is NBL_ERR_UNSUPPORTED (the message names
 *   method 1).  A check above degree 8 is run by one workgroup of max(1, q / 64) waves whose LDS holds the [maxdc][q] inputs, one [q]
 *   vector and two [q] blocks of 16 bytes: (maxdc + 5) q 8 + 256 bytes, at most 76,032 at q = 256 and degree 32, so no shape is refused
 *   for its LDS.  Everything else nbl_create refuses is refused the same way; all of it before the device is touched.
 *   A code whose checks all have degree 8 or less gets exactly the decoder nbl_create / nbl_create_layered_bp would make, the fused
 *   kernels included; on such a code the two layouts evaluate the same operations in the same order and give the same bits.  Every decode
 *   entry point (host, device, bits, samples, prior, csi, idd, resident), soft output (plain and extrinsic), fixed_iters, poll_every and
 *   the active list, the transmitter, channel and error count work unchanged on such a decoder.  nbl_read_state returns post, c2v and v2c
 *   as on the corresponding log-QSPA decoder; nbl_get_layers works on the layered kind.
 *   Every other entry point but nbl_create_fht, nbl_create_fht32_wide, nbl_create_ems_wide and nbl_create_tems_wide keeps its check-degree limit
 *   of 8. */
#define NBL_BP_MAX_CHECK_DEGREE 32
#define NBL_BP_WIDE_LAYERED 1u
nbl_status nbl_create_bp_wide(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                              const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out);

/* ---- Min-Max decoding (method 3): flooding and layered, check degrees up to 32 -------------------------------------------------------
 * The reference names the method (Simulation.h) and has no code for it; this is a decoder kind of this library, defined here operation
 * by operation.  Conventions are the library's: a vector has q slots, slot 0 is 0; L[a] = ln P(a)/P(0), larger = more likely;
 * DecideLLRVector is the decision rule everywhere.
 *
 * The Min-Max check-node update.  Inputs in_0 .. in_{dc-1} with edge coefficients h_d; all arithmetic is IEEE double; inputs are assumed
 * finite.
 *   1. Check domain: p_d[h_d a] = in_d[a], p_d[0] = 0.
 *   2. Dissimilarities: m_d = max_y p_d[y], the slot 0 included, so m_d >= 0; u_d[y] = m_d - p_d[y]: one rounded subtraction, >= +0,
 *      exactly +0 at the maximum.
 *   3. Combination: w_d[y] = min over all (a_k), k != d, with XOR_k a_k = y, of max_{k != d} u_k[a_k].  This is a definition by SET:
 *      evaluation order is immaterial, because min and max select and never round.  The forward / backward recursion with the elementary
 *      step E(A,B)[c] = min_a max(A[a], B[a ^ c]) evaluates it exactly (max(min_i x_i, b) = min_i max(x_i, b)):
 *        F_1 = u_0, F_{k+1} = E(F_k, u_k);   R_{dc-2} = u_{dc-1}, R_{k-1} = E(R_k, u_k);
 *        w_0 = R_0, w_{dc-1} = F_{dc-1}, otherwise w_d = E(F_d, R_d);   for dc = 2: w_0 = u_1, w_1 = u_0.
 *   4. Back to LLRs: c_d[y] = w_d[0] - w_d[y], one rounded subtraction, c_d[0] = 0.
 *   5. Shaping and un-permuting: c2v_d[a] = shape(c_d[h_d a], ems_factor, ems_offset) for a != 0, where shape is what EMS applies to its
 *      c2v values: the identity at factor 1 and offset 0, otherwise divide by the factor (when it is not 1), then the dead zone
 *      (y < -offset: y + offset; y > offset: y - offset; else 0).  nbl_params keeps its layout: Min-Max reads ems_factor / ems_offset and
 *      nothing else of the EMS fields.  ems_factor = 0 is NBL_ERR_ARG (the message names nbl_create_minmax and ems_factor).
 * Every correct evaluation of this update gives the same bits, so parity with a restatement is equality, at every field and degree.
 *
 * Schedules.  Flooding: word for word the reference's EMS iteration (NBLDPC.cpp:805-918) with the update above in place of :859-917 --
 * post in the variable's edge order, decision, syndrome, the freeze at the first zero syndrome, v2c = post - c2v, no damping.  Layered
 * (NBL_MINMAX_LAYERED): word for word the schedule of nbl_create_layered with the same replacement -- the same layer rules,
 * nbl_layer_greedy for layer_of == NULL, the same refusal texts for a bad assignment.
 *
 * nbl_create_minmax: params->method must be NBL_METHOD_MINMAX; any other method is NBL_ERR_UNSUPPORTED (the message names method 3).
 *   flags 0 is flooding (a non-NULL layer_of is NBL_ERR_ARG); an unknown flag bit is NBL_ERR_ARG.  Check degrees 2 .. 32
 *   (NBL_MINMAX_MAX_CHECK_DEGREE; a larger check is NBL_ERR_ARG, the message names this entry point, the degree found and 32); variable
 *   degrees 1 .. 8, with nbl_create's text; q = 4 .. 256; every other refusal of nbl_create holds, with its status and text.  No OSD, no
 *   extension parameters.  All of it before the device is touched.
 *   One programme runs every degree and field under both schedules (nbl_debug_force_generic changes nothing): one check per workgroup of
 *   max(1, q / 64) waves whose LDS holds the [maxdc][q] dissimilarities, two [q] operand blocks and two [q] output vectors:
 *   (maxdc + 4) q 8 bytes, at most 73,728 at q = 256 and degree 32, so no shape is refused for its LDS.
 *   nbl_read_state returns post (with nbl_set_record_state) and c2v; a non-NULL v2c is NBL_ERR_UNSUPPORTED.  nbl_get_layers works on the
 *   layered kind and is NBL_ERR_ARG on the flooding kind.  Every decode entry point (host, device, bits, samples, prior, csi, idd,
 *   resident, noise), soft output (plain and extrinsic), fixed_iters, poll_every and the active list, the transmitter, channel, fading and
 *   error count work unchanged on such a decoder.
 *   nbl_create, nbl_create_ex, nbl_create_osd and the nbl_create_layered* family keep refusing method 3 exactly as before. */
#define NBL_METHOD_MINMAX 3
#define NBL_MINMAX_LAYERED 1u
#define NBL_MINMAX_MAX_CHECK_DEGREE 32
nbl_status nbl_create_minmax(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                             const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out);

/* L_ch: [B][N][q-1] doubles, L_ch[b][n][a-1] = ln P(x_n=a)/P(x_n=0)  (RX_LLR_SYM, Comm.cpp:340-407).
 * out_sym: [B][N] decided symbols (DecodeOutput).  converged: [B] 1 = zero syndrome reached (the
 * reference's return value).  iters: [B] iteration of the first zero syndrome, or max_iter.
 * converged / iters may be NULL. */
nbl_status nbl_decode_batch(nbl_decoder *dec, const double *L_ch, int32_t B, int32_t *out_sym,
                            uint8_t *converged, int32_t *iters);

/* Same, every pointer is DEVICE memory on the decoder's device; work is enqueued on `stream`
 * (a hipStream_t, NULL = the decoder's own stream) and NOT synchronised -- except when poll_every > 0. */
nbl_status nbl_decode_batch_device(nbl_decoder *dec, const double *d_L_ch, int32_t B, int32_t *d_out_sym,
                                   uint8_t *d_converged, int32_t *d_iters, void *stream);

/* ---- device-side soft demodulator: L_ch is built in HBM from the received samples ------------------
 * Replaces CComm::Demodulate (Comm.cpp:340-407) for the two cases the reference implements: BPSK (modOrder == 2, :342-380)
 * and one constellation point per code symbol (modOrder == GFq, :382-398), with the reference's expression order, so
 * the LLRs are bit-identical to the host computation.  Host->device traffic drops from N(q-1) doubles to 2 L doubles per
 * codeword (16x for BPSK GF(256), 128x for 256-QAM).
 * Every other power-of-two order up to 256 (the branch the reference leaves open, Comm.cpp:400-404) runs through the GENERAL
 * demodulator defined below (nbl_set_demodulator_ex). */
typedef struct nbl_demod_desc {
	int32_t mod_order;           /* M = 2^m, 2 <= M <= 256                                               */
	int32_t n_mod_sym;           /* L = received samples per codeword (MOD_SYM_LEN)                      */
	const double *constellation; /* [mod_order][2] (Real, Image) = CONSTELLATION[]; required unless mod_order == 2 on the BPSK path */
	const int32_t *src;          /* mod_order == 2: [N*p] sample index carrying code bit b, -1 = punctured (LLR 0, :350-354)
	                                mod_order == q: [N]   sample index of code symbol n,    -1 = punctured (:386-393)
	                                general path:   [N*p] label-bit index t carrying code bit b, -1 = not transmitted          */
} nbl_demod_desc;
nbl_status nbl_set_demodulator(nbl_decoder *dec, const nbl_demod_desc *demod); /* = nbl_set_demodulator_ex(dec, demod, NULL) */

/* ---- the general demodulator: any M = 2^m, 1 <= m <= 8, against any q = 2^p ------------------------------------------------
 * Nothing in the reference computes these LLRs; the operation is defined here, operation by operation, so that independent
 * implementations agree (tests/demod_general.py restates it in numpy).
 *   Point s of a codeword (s < L) carries label bits (s, i), i = 0 .. m-1; label bit (s, i) has weight 2^(m-1-i) in the
 *   constellation index (CComm::Modulate, Comm.cpp:319).  Linear label-bit index t = s m + i, t < L m.
 *   src [N p]: src[n p + j] = the t that carries bit j (value 2^j) of code symbol n, or -1 when that bit is not transmitted.  Each t
 *   may appear at most once and must be below L m (NBL_ERR_ARG otherwise, checked at the set call before anything is indexed).
 *   Label bits nobody claims are legal and are marginalised; any src (a bit interleaver) is legal, a symbol may touch up to p points.
 *   For symbol n: P(n) = its touched points, ascending s.  For s in P(n) the label positions of s claimed by n are "own", all
 *   others "foreign".
 *   Distance of table point c from the sample (re, im) of point s:   d_s(c) = (re - cr) * (re - cr) + (im - ci) * (im - ci)
 *   C_s(a) = the indices c whose own positions equal the matching bits of value a.
 *   NBL_DEMOD_MAXLOG:  D_s(a) = min of d_s(c) over C_s(a)
 *   NBL_DEMOD_LOGSUM:  dmin = that minimum;
 *                      D_s(a) = dmin - (2 sigma sigma) * log( sum over c in C_s(a), ascending c, of exp( -(d_s(c) - dmin) / (2 sigma sigma) ) )
 *                      (the exact symbol likelihood under uniform foreign bits).  A point without a foreign position has one c
 *                      per a: both metrics are d_s(c) and no exp / log is evaluated.
 *   L[n][a-1] = sum over s in P(n), ascending, accumulated from 0.0, of (D_s(0) - D_s(a)) / (2 sigma sigma);  a = 0 has L = 0;
 *   a symbol without a transmitted bit has all zeros; bits of a that are not transmitted change no C_s.
 * mod_order == 2 and mod_order == q with force_general == 0 take exactly the two paths above (src [N] for mod_order == q);
 * every other order takes the general path, as do these two with force_general == 1 (src [N p] then, constellation required): that
 * flag exists so that the general kernel can be checked against the two reference-pinned ones.
 * NBL_ERR_ARG with a message, before the device is touched: mod_order no power of two, below 2 or above 256; an unknown metric;
 * a general path without constellation.  A refused call leaves the demodulator that was set before usable.
 * Max-log LLRs are bit-identical between this library and the host layer; log-sum LLRs agree to rounding only (device exp / log). */
#define NBL_DEMOD_LOGSUM 0
#define NBL_DEMOD_MAXLOG 1
typedef struct nbl_demod_ext {
	int32_t metric;              /* NBL_DEMOD_*; read by the general path only */
	int32_t force_general;
} nbl_demod_ext;
nbl_status nbl_set_demodulator_ex(nbl_decoder *dec, const nbl_demod_desc *demod, const nbl_demod_ext *ext /* may be NULL: log-sum, not forced */);
/* rx: HOST buffer [B][L][2] (Real, Image) = RX_MOD_SYM after the channel; sigma = sigma_n (Comm.cpp:176-177) */
nbl_status nbl_decode_batch_samples(nbl_decoder *dec, const double *rx, double sigma, int32_t B, int32_t *out_sym,
                                    uint8_t *converged, int32_t *iters);

/* ---- AWGN channel on the device ------------------------------------------------------------------------
 * Replaces CComm::Channel_AWGN (Comm.cpp:328-337) and its noise source CRand (Rand.cpp:17-37) for a batch of lanes: the received
 * samples RX = TX + Rand_Norm(0, sigma) are formed in HBM with the reference's generator and expression order, bit for bit (the
 * log / cos values whose rounding a GPU cannot settle are evaluated by the host's libm inside the call), then demodulated
 * (nbl_set_demodulator must have been called, WITH the constellation points, also for BPSK) and decoded.
 *   tx_index   HOST [B][L] uint8   index into the constellation of every transmitted symbol (CComm::Modulate, Comm.cpp:310-325)
 *   lane_state HOST [B][3] uint32  IX, IY, IZ of each lane's CRand before the frame's first draw
 * The frame consumes 4 L uniform draws per lane (real and imaginary part of every symbol, two draws each); the caller moves
 * its copy of each lane's generator on with nbl_rand_advance(state, 4 L). */
nbl_status nbl_decode_batch_noise(nbl_decoder *dec, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int32_t B,
                                  int32_t *out_sym, uint8_t *converged, int32_t *iters);
/* The same in two phases, for callers that overlap the channel of batch k+1 with the decode of batch k (two host threads):
 * nbl_channel_batch forms the samples of a batch into the decoder's resident buffer `slot` (0 or 1) on a second stream and returns
 * when they are complete; nbl_decode_batch_resident demodulates and decodes what a slot holds.  A channel call and a decode call
 * on DIFFERENT slots may run concurrently; otherwise the handle is single-threaded like every other call.  The two threads keep
 * separate error texts (nbl_last_error reports the decode side's, then the channel side's after " | channel: ").
 * tx_index values must be below mod_order (NBL_ERR_ARG otherwise). */
nbl_status nbl_channel_batch(nbl_decoder *dec, int32_t slot, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int32_t B);
nbl_status nbl_decode_batch_resident(nbl_decoder *dec, int32_t slot, double sigma, int32_t B, int32_t *out_sym, uint8_t *converged,
                                     int32_t *iters);
/* state <- state after `draws` calls of CRand::Rand_Uniform (Rand.cpp:17-28); pure host arithmetic */
void nbl_rand_advance(uint32_t state[3], uint64_t draws);

/* ---- transmit side and error count on the device --------------------------------------------------------------------------
 * Replaces, for a batch of lanes, CComm::GenerateMessage (PN register, Comm.cpp:181-252), CRCEncode (:506-561), CNBLDPC::Encode
 * (NBLDPC.cpp:562-604), the symbol -> bit unpacking, Puncture and Modulate (Comm.cpp:255-325) and, after the decode, TakeDecoded +
 * Err (Comm.cpp:421-493).  Legal after nbl_set_demodulator WITH the constellation points.
 *   gen        [N][K] uint16, K = N - M: the encoder as a dense linear map, code[n] = sum_k gen[n][k] * msg[k] over GF(q), the final
 *              column exchanges of CNBLDPC::Encode (NBLDPC.cpp:588-597) included.  H * gen = 0 is checked on the host with the
 *              decoder's own graph and tables (NBL_ERR_ARG otherwise).  May be NULL when random_msg == 0.
 *   crc_len    sim.crcLen: 0, 8, 16 or 24 (NBL_ERR_ARG otherwise); above K p: NBL_ERR_UNSUPPORTED
 *   random_msg sim.randomMsg: 0 = all-zero message AND all-zero codeword, encoder skipped (Comm.cpp:258-268)
 *   parallel   sim.parallel, the PN stride: every message bit costs `parallel` clocks of the register (Comm.cpp:201-202)
 *   punct      [n_punct] punctured symbol positions, ascending (Comm.cpp:290-308)
 *   mod_order, n_mod_sym   must repeat the demodulator's (NBL_ERR_ARG otherwise); mod_order above 256 is NBL_ERR_UNSUPPORTED
 * Shapes the kernels do not serve (N p above 65536 bits, a matrix above 64 MiB) are NBL_ERR_UNSUPPORTED at this call. */
typedef struct nbl_tx_desc {
	const uint16_t *gen;
	int32_t crc_len, random_msg, parallel;
	const int32_t *punct;
	int32_t n_punct;
	int32_t mod_order, n_mod_sym;
} nbl_tx_desc;
nbl_status nbl_set_transmitter(nbl_decoder *dec, const nbl_tx_desc *tx);
/* nbl_channel_batch with tx_index produced on the device (same slots, same second stream, same threading contract).
 *   pn_state   HOST [B] uint16: each lane's 11-bit PN register in front of the frame, bit i = regPN[i].  The frame consumes
 *              (K p - crc_len) * parallel clocks when random_msg != 0 (none otherwise); the caller moves its copy on with nbl_pn_advance.
 *   lane_state as nbl_channel_batch
 * The slot keeps, on the device, the code word and with it the transmitted message AS Encode LEAVES IT: the first K code symbols
 * after the exchanges (NBLDPC.cpp:598-601, Comm.cpp:281-285) -- what Err compares against, not the PN draw. */
nbl_status nbl_transmit_batch(nbl_decoder *dec, int32_t slot, const uint16_t *pn_state, const uint32_t *lane_state, double sigma, int32_t B);
/* state <- the register after `clocks` calls of GenPN (Comm.cpp:241-252); pure host arithmetic */
void nbl_pn_advance(uint16_t *state, uint64_t clocks);
/* Comm.cpp:421-493 per lane, between the outputs of the last nbl_decode_batch_resident on `slot` (kept on the device once a
 * transmitter is set) and the slot's transmitted message.  HOST arrays [B]: err_sym, err_bit (message part only), crc_ok =
 * CrcCheck(RX_MSG_BIT, K p, crc_len, 1) literally: polynomial type 1 for CRC-24 (the encoder used type 0), 1 when crc_len == 0, 0 for
 * an all-zero word.  With a transmitter set, nbl_decode_batch_resident accepts out_sym == NULL. */
nbl_status nbl_count_errors(nbl_decoder *dec, int32_t slot, int32_t B, int32_t *err_sym, int32_t *err_bit, uint8_t *crc_ok);
/* The plain encoder (host buffers): code [B][N] = gen * msg [B][K]; msg_out (may be NULL) = the first K code symbols. */
nbl_status nbl_encode_batch(nbl_decoder *dec, const int32_t *msg, int32_t B, int32_t *code, int32_t *msg_out);
/* What a slot holds for lanes b0 .. b0 + n - 1 (any pointer may be NULL): tx_msg [n][K], tx_code [n][N] int32, tx_index [n][L]
 * uint8.  For parity tests. */
nbl_status nbl_read_transmitted(nbl_decoder *dec, int32_t slot, int32_t b0, int32_t n, int32_t *tx_msg, int32_t *tx_code, uint8_t *tx_index);

/* ---- bit-LLR input and batched soft output ------------------------------------------------------------------------------------
 * Bit <-> symbol LLR conversion around the message-passing core, per batch, on the device: for callers whose front end is not one of
 * ours (an equaliser, an OFDM demapper, a fading channel) and for receivers that iterate around the decoder (turbo equalisation,
 * iterative demapping, an outer code).  Defined here operation by operation, so that independent implementations agree
 * (tests/soft_ref.py restates it in numpy).
 *   A bit LLR is ln P(bit = 1) / P(bit = 0) -- the sign of the reference's RX_LLR_BIT.  Bit j of symbol a has value 2^j; q = 2^p.
 *
 * Bit-LLR input.  lam is [B][N p] doubles.  For every variable n and every a = 1 .. q-1:
 *     s = 0.0;  for j = 0 .. p-1 ascending: if ((a >> j) & 1) s = s + lam[n p + j];  L_ch[n][a-1] = s
 *   (Comm.cpp:362-372, which accumulates from 0).  Nothing else is done to the values; a punctured bit is the caller's 0.0.
 *   nbl_decode_batch_bits / nbl_decode_batch_bits_device behave exactly as nbl_decode_batch / nbl_decode_batch_device on the expanded
 *   L_ch: the same stream and synchronisation contract (the device form is enqueued on `stream` and not synchronised, except when
 *   poll_every > 0), the same argument checks (NBL_ERR_ARG for a NULL decoder, input or out_sym, or B < 0; B == 0 is NBL_OK), on every
 *   decoder kind: flooding, layered, layered-damped, nbl_create_ex, nbl_create_osd, and method 6 (which reads L_ch only).  No
 *   demodulator has to be set.  Host -> device traffic is N p doubles per codeword instead of N (q - 1).
 *
 * Soft output of the LAST decode call (any of the decode entry points), for all B codewords of that call.
 *   For codeword b let c2v be exactly what nbl_read_state returns for b, the reference's L_c2v at return: under early exit
 *   (fixed_iters == 0) a codeword that converged at iteration k has the messages of iteration k-1 (zeros for k = 1); in every other
 *   case the messages as the last iteration left them.  Then
 *     P[n] = L_ch[n], then += c2v[e] for each edge e of n in n's edge order (AddLLRVector, the expression of NBLDPC.cpp:678-685);
 *     P[n][0] = 0.
 *     sym_llr[b][n][a-1] = P[n][a]
 *     for bit j of n:  S1 = {a : (a >> j) & 1},  S0 = the rest, a = 0 (value 0.0) included;  M1 = max over S1,  M0 = max over S0
 *       NBL_SOFT_MAXLOG:  bit_llr[b][n p + j] = M1 - M0
 *       NBL_SOFT_LOGSUM:  bit_llr[b][n p + j] = (M1 + log(sum over S1, ascending a, of exp(P[a] - M1)))
 *                                               - (M0 + log(sum over S0, ascending a, of exp(P[a] - M0)))
 *       A difference that is zero is returned as +0.0 (the value written is the difference + 0.0), so the sign of a zero among the
 *       P[a] never shows.
 *   Max-log values are bit-identical between implementations; log-sum values agree to rounding only (device exp / log, and a tree
 *   reduction where the definition sums in sequence).
 *   Consequences:
 *     - For a codeword that converged under early exit, P is the reference's L_post at return and DecideLLRVector(P[n]) == out_sym[n].
 *     - For a codeword that did not converge, P is one check-node pass NEWER than the decision in out_sym (the reference, too, leaves
 *       its loop after the check-node pass of the last iteration).
 *     - With fixed_iters = 1, P is the state after max_iter iterations for every codeword, converged or not.
 *     - OSD post-processing changes out_sym only, never the soft output.
 *     - These are a-posteriori values.  Symbol-level extrinsic values are nbl_soft_output_ex's (below).
 *     - max_iter = 0 is legal: P = L_ch.
 *   sym_llr [B][N][q-1] and bit_llr [B][N p]; either may be NULL (then it is not written), not both.
 *   nbl_soft_output: host buffers; returns when they are filled.  nbl_soft_output_device: device buffers on the decoder's device; the
 *   work is enqueued on `stream` (NULL = the decoder's own) and NOT synchronised; the caller orders it behind the decode: the same
 *   stream, or poll_every > 0, which has synchronised already.  Nothing the call needs is read back to the host.
 *   Refused with a message: NBL_ERR_ARG for both pointers NULL, an unknown metric, or no decode call on this handle yet;
 *   NBL_ERR_UNSUPPORTED on a method-6 decoder (it runs no iterations: there are no messages).
 *   Costs nothing unless called; needs neither nbl_set_record_state nor any other preparation. */
nbl_status nbl_decode_batch_bits(nbl_decoder *dec, const double *bit_llr /* HOST [B][N p] */, int32_t B, int32_t *out_sym,
                                 uint8_t *converged, int32_t *iters);
nbl_status nbl_decode_batch_bits_device(nbl_decoder *dec, const double *d_bit_llr, int32_t B, int32_t *d_out_sym, uint8_t *d_converged,
                                        int32_t *d_iters, void *stream);
#define NBL_SOFT_LOGSUM 0
#define NBL_SOFT_MAXLOG 1
nbl_status nbl_soft_output(nbl_decoder *dec, int32_t metric, double *sym_llr /* HOST [B][N][q-1] or NULL */,
                           double *bit_llr /* HOST [B][N p] or NULL */);
nbl_status nbl_soft_output_device(nbl_decoder *dec, int32_t metric, double *d_sym_llr, double *d_bit_llr, void *stream);

/* ---- iterative demapping: bit priors for the general demodulator, extrinsic soft output, and the loop between them -----------------
 * A receiver whose constellation does not match the field (M != q) can feed the decoder's knowledge of the OTHER symbols' bits back
 * into the demodulator (BICM-ID).  Nothing in the reference computes any of this; the operations are defined here, operation by
 * operation, so that independent implementations agree (tests/idd_ref.py restates them in numpy, with a probability-domain brute
 * force beside the demodulator).  Sign and bit order are the soft output's: a bit LLR is
 * ln P(bit = 1) / P(bit = 0), bit j of symbol a has value 2^j.
 *
 * Prior-aware general demodulator.  prior is [B][N p] doubles, indexed by code bit g = n p + j.  Everything of the general
 * demodulator above stays; only the distance of table point c at point s, as seen by symbol n, changes:
 *     A_s,n(c) = 0.0;  for label position i = 0 .. m-1 ascending:
 *                    if i is foreign to n at s, AND some code bit g claims label bit t = s m + i (src[g] == t), AND bit i of c
 *                    (weight 2^(m-1-i)) is 1:   A = A + prior[b][g]
 *     d'_s,n(c) = d_s(c) - (2 sigma sigma) * A_s,n(c)
 *   d' replaces d in both metrics: the minimum, the dmin of log-sum, and the exponent.  Own positions never contribute, so the result
 *   is extrinsic with respect to symbol n's own bits; unclaimed label bits stay uniform; a prior of all 0.0 gives d' = d exactly and
 *   LLRs bit-identical to the prior-less path.  Non-finite priors are the caller's problem.
 *   nbl_decode_batch_samples_prior: nbl_decode_batch_samples with that demodulator.  prior == NULL IS nbl_decode_batch_samples and
 *   launches the kernel that call launches.  A BPSK or q-ary demodulator that is not forced general has no foreign position: a prior
 *   is accepted and inert there.
 *
 * Extrinsic soft output.  nbl_soft_output_ex / nbl_soft_output_device_ex with flags == 0 ARE nbl_soft_output / nbl_soft_output_device.
 *   NBL_SOFT_EXTRINSIC: P[n] starts from the all-0.0 vector instead of L_ch[n]; everything else of the soft output's definition holds
 *   word for word -- the choice of c2v per codeword, the edge order, the +0.0 rule -- on every decoder kind the existing call works
 *   on, with the same refusals plus NBL_ERR_ARG for an unknown flag bit.  (The bit marginals of the symbol-level extrinsic cannot be
 *   had by subtracting bit LLRs, hence the call.)
 *
 * The loop.  Per codeword b, independently of every other codeword of the batch:
 *     prior_1 = all 0.0
 *     for k = 1 .. passes:
 *         L_ch = the prior-aware demodulator of b's samples with prior_k
 *         decode exactly as one nbl_decode_batch_samples call does from that L_ch (messages start from zero; max_iter, fixed_iters,
 *             poll_every, OSD as the decoder was created)
 *         if converged, or k == passes:  out_sym, converged, iters are this pass's;  passes_used[b] = k;  stop
 *         prior_{k+1} = the extrinsic bit LLRs (NBL_SOFT_EXTRINSIC, soft_metric) of this pass's state
 *   passes == 1 IS the plain call, bit for bit.  Passes 2 and later run on the codewords still unconverged only, gathered into dense
 *   buffers, with grids sized to them; the survivor count is read back after every pass that has a successor: ONE host
 *   synchronisation per pass, also where poll_every == 0.  The caller's samples and a slot's samples are never overwritten.
 *   With max-log metrics on both sides every output is bit-identical between implementations; under log-sum one rounding can flip a
 *   convergence, so only a single pass from a given prior is comparable.
 *   nbl_decode_batch_samples_idd: host samples, as nbl_decode_batch_samples.  nbl_decode_batch_resident_idd: the samples a slot
 *   holds, as nbl_decode_batch_resident; it leaves the final words where nbl_count_errors reads them and out_sym may be NULL once a
 *   transmitter is set.  passes_used [B] may be NULL.
 *   Refused with a message, before the device is touched: NBL_ERR_ARG for a NULL idd, passes < 1, an unknown soft_metric, or no
 *   demodulator set; NBL_ERR_UNSUPPORTED for passes > 1 on a method-6 decoder (it has no messages).  On a BPSK or q-ary demodulator
 *   that is not forced general the later passes are provably the same decode: pass 1 runs alone and a codeword that did not converge
 *   reports passes_used = passes.
 *   After a loop call with passes > 1 on a general demodulator the workspace holds a sub-batch: until the next ordinary decode call
 *   nbl_soft_output* and nbl_read_state are refused (NBL_ERR_ARG, the message says why), and nbl_last_timing describes the last
 *   pass's sub-batch decode alone, not the call.  A plain decode afterwards behaves as if the loop call had never happened.  The loop's buffers grow on demand and count in nbl_workspace_bytes. */
#define NBL_SOFT_EXTRINSIC 1u
typedef struct nbl_idd_params {
	int32_t passes;              /* >= 1 */
	int32_t soft_metric;         /* NBL_SOFT_*: the metric of the extrinsic bit LLRs between passes */
} nbl_idd_params;
nbl_status nbl_decode_batch_samples_prior(nbl_decoder *dec, const double *rx, const double *prior /* HOST [B][N p] or NULL */, double sigma,
                                          int32_t B, int32_t *out_sym, uint8_t *converged, int32_t *iters);
nbl_status nbl_soft_output_ex(nbl_decoder *dec, int32_t metric, uint32_t flags, double *sym_llr, double *bit_llr);
nbl_status nbl_soft_output_device_ex(nbl_decoder *dec, int32_t metric, uint32_t flags, double *d_sym_llr, double *d_bit_llr, void *stream);
nbl_status nbl_decode_batch_samples_idd(nbl_decoder *dec, const double *rx, double sigma, int32_t B, const nbl_idd_params *idd,
                                        int32_t *out_sym, uint8_t *converged, int32_t *iters, int32_t *passes_used /* [B] or NULL */);
nbl_status nbl_decode_batch_resident_idd(nbl_decoder *dec, int32_t slot, double sigma, int32_t B, const nbl_idd_params *idd,
                                         int32_t *out_sym, uint8_t *converged, int32_t *iters, int32_t *passes_used /* [B] or NULL */);

/* ---- flat fading: per-sample channel gains in the demodulators, Rayleigh block fading on the device ---------------------------------
 * Coherent reception of y = h x + n with a known complex gain h per received sample.  Nothing in the reference computes any of this;
 * the operations are defined here, operation by operation, so that independent implementations agree (tests/fading_ref.py restates
 * them in numpy, with a probability-domain brute force beside the general demodulator).  All arithmetic is IEEE
 * double; each product and each sum is rounded on its own, no contraction.
 *
 * Gains.  gain is [B][L][2] doubles (Real, Image), laid out like rx: one gain per received sample.
 * Faded point.  For sample s with gain (hr, hi) and table point c = (cr, ci):
 *     pr = hr * cr - hi * ci
 *     pi = hr * ci + hi * cr
 * Demodulators with gains.
 *   General path:  d_s(c) = (re - pr) * (re - pr) + (im - pi) * (im - pi).  Everything else of the general demodulator's definition
 *     holds word for word: own and foreign positions, C_s(a), max-log and log-sum, the prior term d' = d - (2 sigma sigma) * A, the
 *     ascending orders.
 *   One point per symbol (mod_order == q, not forced general): the existing expression with the faded points of sample s = src[n]
 *     (p0 of table point 0, pa of table point a) in place of the table's:
 *       num = (2 * re - p0r - par) * (par - p0r) + (2 * im - p0i - pai) * (pai - p0i);   L = num / (2 * sigma * sigma)
 *   BPSK path:  z = hr * re + hi * im, and the bit LLR is -2 * z / (sigma * sigma): the existing expression with z in place of re.
 *     Punctured bits stay 0.0.
 *   Consequences:
 *     - A gain of (1, 0) everywhere gives LLRs equal as numbers to the gain-less call's; only the sign of a zero may differ.
 *     - On the general and q-ary paths a gain that is constant over a frame gives LLRs bit-identical to the gain-less demodulator set
 *       up with the pre-faded table (pr, pi).
 *     - On the BPSK path a real positive gain g gives the gain-less demodulator's LLRs for samples g * re.
 *   nbl_decode_batch_samples_csi: nbl_decode_batch_samples_prior with that demodulator.  gain == NULL IS nbl_decode_batch_samples_prior
 *   and launches the kernel that call launches.  nbl_decode_batch_samples_idd_csi: the loop of nbl_decode_batch_samples_idd with the
 *   gain-aware demodulator in every pass; when passes 2 and later gather the unconverged codewords into dense buffers, their gains are
 *   gathered with them.  gain == NULL IS nbl_decode_batch_samples_idd.  Both refuse what the calls they extend refuse.
 *
 * Rayleigh block fading on the device.  nbl_set_fading(dec, f): model NBL_FADING_NONE or NBL_FADING_RAYLEIGH; coherence >= 1 = the
 *   number of consecutive samples that share one gain.  f == NULL or NONE gives AWGN again, exactly as before the call.  An unknown
 *   model or coherence < 1 is NBL_ERR_ARG with a message; a refused call leaves the previous setting in force.  Legal any time after
 *   creation; it survives nbl_set_demodulator*, the block count follows the current L.
 *   With Rayleigh set, a frame of a lane is formed in this order:
 *     1. nblk = ceil(L / coherence)
 *     2. for block k = 0 .. nblk-1, in order, with S = sqrt(0.5) as a double:  hr_k = Rand_Norm(0, S);  hi_k = Rand_Norm(0, S)
 *        (four uniform draws per block, Rand.cpp:31-37's expression order)
 *     3. the noise exactly as Channel_AWGN draws it (Comm.cpp:328-337): nr, ni per sample, 4 L uniform draws
 *     4. for sample s, k = s / coherence, transmitted point (cr, ci):
 *          RX.Real  = (hr_k * cr - hi_k * ci) + nr
 *          RX.Image = (hr_k * ci + hi_k * cr) + ni
 *   A frame therefore moves a lane's generator 4 nblk + 4 L draws: nbl_channel_draws(dec) returns that number, 4 L without fading
 *   (0 before a demodulator is set).  E|h|^2 = 1, so the Eb/N0 -> sigma relation stays as it is.
 *   With Rayleigh set nbl_decode_batch_noise, nbl_channel_batch and nbl_transmit_batch form faded samples and keep the per-sample
 *   gains beside the samples -- in a slot they stay resident, one buffer per slot, grown on demand and counted in
 *   nbl_workspace_bytes -- and nbl_decode_batch_noise, nbl_decode_batch_resident and nbl_decode_batch_resident_idd demodulate with
 *   those gains.  A slot remembers whether it holds gains: a slot filled before nbl_set_fading decodes as AWGN.
 *   nbl_read_gains: the gains [n][L][2] a slot holds for lanes b0 .. b0 + n - 1, for parity tests; NBL_ERR_ARG on a slot without gains.
 * Out of scope: a per-sample noise variance, non-coherent reception, channel estimation, frequency-selective channels. */
#define NBL_FADING_NONE 0
#define NBL_FADING_RAYLEIGH 1
typedef struct nbl_fading_desc {
	int32_t model;               /* NBL_FADING_* */
	int32_t coherence;           /* >= 1: consecutive samples that share one gain */
} nbl_fading_desc;
nbl_status nbl_decode_batch_samples_csi(nbl_decoder *dec, const double *rx, const double *gain /* HOST [B][L][2] or NULL */,
                                        const double *prior /* HOST [B][N p] or NULL */, double sigma, int32_t B, int32_t *out_sym,
                                        uint8_t *converged, int32_t *iters);
nbl_status nbl_decode_batch_samples_idd_csi(nbl_decoder *dec, const double *rx, const double *gain /* HOST [B][L][2] or NULL */, double sigma,
                                            int32_t B, const nbl_idd_params *idd, int32_t *out_sym, uint8_t *converged, int32_t *iters,
                                            int32_t *passes_used /* [B] or NULL */);
nbl_status nbl_set_fading(nbl_decoder *dec, const nbl_fading_desc *f /* NULL: AWGN */);
uint64_t nbl_channel_draws(const nbl_decoder *dec);
nbl_status nbl_read_gains(nbl_decoder *dec, int32_t slot, int32_t b0, int32_t n, double *gain /* HOST [n][L][2] */);

/* Message state of codeword b after the last decode call (host buffers, any may be NULL):
 * post [N][q-1], v2c [E][q-1], c2v [E][q-1], edges in variable-major order.  For parity tests.
 * post and c2v are the reference's members at return.  v2c differs for a codeword that CONVERGED at iteration k >= 2: the
 * variable-node pass writes the messages of iteration k before the syndrome is known, the reference returns with those of
 * iteration k-1 (NBLDPC.cpp:693-715 precedes :718-744); they are never used afterwards.  In fixed-iteration mode (timing)
 * the message buffers of a converged codeword keep being updated; only its outputs are frozen. */
nbl_status nbl_read_state(nbl_decoder *dec, int32_t b, double *post, double *v2c, double *c2v);

/* Keep L_post of the last variable-node pass so nbl_read_state can return it (costs N q-vectors of
 * extra HBM writes per iteration; off by default). */
nbl_status nbl_set_record_state(nbl_decoder *dec, int32_t on);

/* Per-phase device time of the last decode call in milliseconds (HIP events on the launch stream):
 * ms[0] variable-node kernels, ms[1] syndrome kernels, ms[2] check-node kernels, ms[3] whole call.
 * Only filled when profiling was switched on with nbl_set_profiling(dec, 1).
 * launches[0..2]: variable-node, syndrome and check-node launches of the last decode call.  Undamped fused EMS leaves the check-node
 * pass of iteration max_iter, which no output of the call depends on, to the first nbl_read_state / nbl_soft_output* that asks for
 * the messages: a profiled call counts the launches its times cover (max_iter - 1 until that pass has run), an unprofiled one the
 * passes of its schedule (max_iter). */
nbl_status nbl_set_profiling(nbl_decoder *dec, int32_t on);
nbl_status nbl_last_timing(nbl_decoder *dec, double ms[4], int64_t launches[3]);

int32_t nbl_abi_version(void);
const char *nbl_last_error(const nbl_decoder *dec); /* dec may be NULL: error of the last failed nbl_create */
size_t nbl_workspace_bytes(const nbl_decoder *dec);

#ifdef __cplusplus
}
#endif
#endif
