// nbldpc_amd/csrc/nbl_api.cpp -- C ABI (include/nbldpc.h) on top of the HIP kernels.
//
// This unit: the workspace, the iteration loop, nbl_decode_batch*, state read-back and the debug switches (nbl_decoder.h maps the rest).
// Replaces CNBLDPC::Decoding's iteration loop (NBLDPC.cpp:607-641 -> Decoding_BP/EMS/TEMS/BS_TEMS) for a batch of codewords.
#include <cstdlib>
#include <cstring>
#include "nbl_decoder.h"
#include "nbl_tems_path.h"

thread_local std::string g_create_error;

static void drop_graphs(nbl_decoder *d)
{
	for (auto &ge : d->gexec)
		if (ge) (void)hipGraphExecDestroy(ge);
	d->gexec.clear();
	d->pending.on = false; // (the buffers a pending pass names go with what is dropped here: it is never run late)
}

static void free_workspace(nbl_decoder *d)
{
	drop_graphs(d);
	d->ws = nbl_decoder::Ws(); // (every buffer of the old one is released)
	d->w.Lch = d->w.v2c = d->w.c2v = d->w.post = nullptr;
	d->w.dec = d->w.out = d->w.iters = d->w.edge_dec = nullptr;
	d->w.done = nullptr;
	d->w.active = nullptr;
	d->w32 = NblWork32{};
	d->wide_valid = false;
	d->cap = 0;
	d->last_B = 0; // (nothing of the last decode call is left to read)
	d->last_c2v = nullptr;
}

static bool small_enabled()
{
	static const bool on = !getenv("NBL_NO_SMALL"); // A/B measurements: the several-checks-per-wave kernels on small fields
	return on;
}

// The kernel choice of this decoder as it stands (nbl_plan.cpp): once per workspace check and once per decode, never per launch
static NblPlan plan_of(const nbl_decoder *d)
{
	return nbl_plan(d->shape, d->prm, NblPlanReq{d->kind, d->layered, d->force_generic, d->record_state, small_enabled()});
}

// nbl_create_fht32 / nbl_create_fht32_wide: the FP64 L_ch every front end fills, the float state the iterations run on, decisions and flags.  The FP64 c2v /
// v2c / post are not made here (widen_state makes them for the first FP64 reader of the state).
static nbl_status ensure_workspace32(nbl_decoder *d, int B)
{
	const bool want_post = d->record_state;
	if (B <= d->cap && (!want_post || d->w32.post)) return NBL_OK;
	const int cap = B > d->cap ? B : d->cap;
	free_workspace(d);
	const size_t q = d->g.q, N = d->g.N, E = d->g.E;
	nbl_decoder::Ws &b = d->ws;
	nbl_status s = NBL_OK;
	auto make = [&](auto &buf, bool want, size_t n) { if (!s && want) s = buf.grow(d->err, n); };
	make(b.Lch, true, (size_t)cap * N * q * 8);
	make(b.Lf, true, (size_t)cap * N * q * 4);
	make(b.v2c32, true, (size_t)cap * E * q * 4);
	make(b.c2v32, true, (size_t)cap * E * q * 4);
	make(b.post32, want_post, (size_t)cap * N * q * 4);
	make(b.dec, true, (size_t)cap * N * 4);
	make(b.out, true, (size_t)cap * N * 4);
	make(b.iters, true, (size_t)cap * 4);
	make(b.done, true, (size_t)cap);
	make(b.active, true, (size_t)cap * 4);
	if (s) { free_workspace(d); return s; }
	d->w.Lch = b.Lch;
	d->w.dec = b.dec; d->w.out = b.out; d->w.iters = b.iters; d->w.done = b.done;
	d->w32 = NblWork32{b.Lf, b.v2c32, b.c2v32, b.post32};
	d->cap = cap;
	return NBL_OK;
}

nbl_status widen_state(nbl_decoder *d, hipStream_t reader)
{
	if (!nbl_kind_f32(d->kind) || d->last_B <= 0 || !d->w32.c2v) return NBL_OK;
	hipStream_t st = reader ? reader : d->stream;
	if (d->wide_valid && d->wide_stream == st) return NBL_OK;
	const size_t q = d->g.q, N = d->g.N, E = d->g.E, cap = (size_t)d->cap;
	nbl_decoder::Ws &b = d->ws;
	nbl_status s;
	if ((s = b.c2v.grow(d->err, cap * E * q * 8)) || (s = b.v2c.grow(d->err, cap * E * q * 8))) return s;
	if (d->w32.post && (s = b.post.grow(d->err, cap * N * q * 8))) return s;
	d->w.c2v = b.c2v; d->w.v2c = b.v2c;
	d->w.post = d->w32.post ? b.post.p : nullptr; // (what the last decode did not record is not read: nbl_read_state's rule)
	d->last_c2v = d->w.c2v;
	const long long B = d->last_B;
	HIP_TRY(d, nbl_launch_widen32(d->w32.c2v, d->w.c2v, B * (long long)(E * q), st));
	HIP_TRY(d, nbl_launch_widen32(d->w32.v2c, d->w.v2c, B * (long long)(E * q), st));
	if (d->w.post) HIP_TRY(d, nbl_launch_widen32(d->w32.post, d->w.post, B * (long long)(N * q), st));
	d->wide_valid = true;
	d->wide_stream = st;
	return NBL_OK;
}

nbl_status ensure_workspace(nbl_decoder *d, int B)
{
	const NblPlan plan = plan_of(d);
	if (plan.f32) return ensure_workspace32(d, B);
	const bool want_v2c = plan.want_v2c;
	const bool want_post = d->record_state || d->osd_acc;
	if (B <= d->cap && (!want_post || d->w.post) && (!want_v2c || d->w.v2c)) return NBL_OK;
	int cap = B > d->cap ? B : d->cap;
	free_workspace(d);
	const size_t q = d->g.q, N = d->g.N, E = d->g.E;
	nbl_decoder::Ws &b = d->ws;
	nbl_status s = NBL_OK;
	auto make = [&](auto &buf, bool want, size_t n) { if (!s && want) s = buf.grow(d->err, n); };
	make(b.Lch, true, (size_t)cap * N * q * 8);
	make(b.v2c, want_v2c, (size_t)cap * E * q * 8);
	make(b.c2v, true, (size_t)cap * E * q * 8);
	// (fusable, whatever force_generic says: nbl_workspace_bytes does not move with a debug switch)
	make(b.c2v_alt, plan.fusable, (size_t)cap * E * q * 8);
	make(b.c2v_zero, plan.fusable, E * q * 8); // one block for every codeword (NblWork::c2v_prev_shared)
	auto clear_zero = [&]() -> nbl_status { HIP_TRY(d, hipMemset(b.c2v_zero, 0, E * q * 8)); return NBL_OK; };
	if (!s && plan.fusable) s = clear_zero();
	make(b.post, want_post, (size_t)cap * N * q * 8);
	make(b.osd_S, d->osd_acc, (size_t)cap * N * d->g.p * 8);
	make(b.dec, true, (size_t)cap * N * 4);
	make(b.edge_dec, d->prm.method != NBL_METHOD_EMS && d->kind != NBL_KIND_MINMAX, (size_t)cap * E * 4); // (the damped methods' state)
	make(b.out, true, (size_t)cap * N * 4);
	make(b.iters, true, (size_t)cap * 4);
	make(b.done, true, (size_t)cap);
	make(b.active, true, (size_t)cap * 4);
	if (s) { free_workspace(d); return s; } // (a workspace is whole or absent: nbl_workspace_bytes counts nothing of a failed one)
	d->w.Lch = b.Lch; d->w.v2c = b.v2c; d->w.c2v = b.c2v; d->w.post = b.post;
	d->w.dec = b.dec; d->w.edge_dec = b.edge_dec; d->w.out = b.out; d->w.iters = b.iters; d->w.done = b.done;
	d->cap = cap;
	return NBL_OK;
}

extern "C" int32_t nbl_abi_version(void) { return NBL_ABI_VERSION; }

extern "C" const char *nbl_last_error(const nbl_decoder *dec)
{
	if (!dec) return g_create_error.c_str();
	if (dec->err2.empty()) return dec->err.c_str();
	if (dec->err.empty()) return dec->err2.c_str();
	static thread_local std::string both;
	both = dec->err + " | channel: " + dec->err2;
	return both.c_str();
}

// the workspace, the staging buffers of priors, bit LLRs and soft output, the buffers of the demapping loop, and the gains
extern "C" size_t nbl_workspace_bytes(const nbl_decoder *dec)
{
	if (!dec) return 0;
	return dec->ws.bytes() + dec->d_prior.size + dec->d_lam.size + dec->d_soft_sym.size + dec->d_soft_bit.size + dec->idd.bytes() + dec->d_gain.size +
	       dec->d_gains[0].size + dec->d_gains[1].size;
}

extern "C" void nbl_destroy(nbl_decoder *d)
{
	if (!d) return;
	if (d->device >= 0) (void)hipSetDevice(d->device);
	if (d->stream) { (void)hipStreamSynchronize(d->stream); }
	(void)hipDeviceSynchronize(); // graphs may still be running on a caller's stream
	if (d->stream2) (void)hipStreamSynchronize(d->stream2);
	drop_graphs(d);
	for (void *p : d->graph_allocs) (void)hipFree(p);
	if (d->stream2) (void)hipStreamDestroy(d->stream2);
	for (auto &e : d->ev)
		if (e) (void)hipEventDestroy(e);
	for (auto &e : d->pev) (void)hipEventDestroy(e);
	if (d->pending_ev) (void)hipEventDestroy(d->pending_ev);
	if (d->stream) (void)hipStreamDestroy(d->stream);
	delete d; // (every buffer the handle owns is freed by its DevBuf)
}

extern "C" nbl_status nbl_set_profiling(nbl_decoder *d, int32_t on)
{
	if (!d) return NBL_ERR_ARG;
	d->profiling = on != 0;
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): route every shape through the generic kernels (1), the specialised ones without the
// fused iteration (2); on an nbl_create_fht decoder 3 selects the wide programme (nbl_cn_fht_wide.hip) at any check degree, on an
// nbl_create_ems_wide decoder the workgroup-per-check programme (nbl_cn_ems_wide.hip), on an nbl_create_tems_wide decoder with
// tems_nc <= NBL_TEMS_WIDE_MAX_NC that of nbl_cn_tems_wide.hip, on an nbl_create_bp_wide decoder that of nbl_cn_bp_wide.hip, on an
// nbl_create_fht32_wide decoder that of nbl_cn_fht32_wide.hip.  An nbl_create_minmax decoder has one programme: no value moves it.
extern "C" nbl_status nbl_debug_force_generic(nbl_decoder *d, int32_t on)
{
	if (!d) return NBL_ERR_ARG;
	d->force_generic = on;
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): number of iteration windows currently held as executable hipGraphs
extern "C" int32_t nbl_debug_graph_windows(nbl_decoder *d)
{
	int n = 0;
	if (d)
		for (auto &ge : d->gexec) n += ge != nullptr;
	return n;
}

// Diagnostic only (not part of include/nbldpc.h): in-kernel cycle stamps of the check-node kernel.
extern "C" nbl_status nbl_debug_stamps(nbl_decoder *d, int32_t on, unsigned long long out[NBL_STAMP_SLOTS])
{
	if (!d) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	if (out && d->w.stamps) {
		HIP_TRY(d, hipStreamSynchronize(d->stream));
		HIP_TRY(d, hipDeviceSynchronize());
		HIP_TRY(d, hipMemcpy(out, d->w.stamps, NBL_STAMP_SLOTS * 8, hipMemcpyDeviceToHost));
	}
	if (on && !d->w.stamps) {
		void *p = nullptr;
		HIP_TRY(d, hipMalloc(&p, NBL_STAMP_SLOTS * 8));
		d->graph_allocs.push_back(p);
		d->w.stamps = (unsigned long long *)p;
	}
	if (d->w.stamps && on) HIP_TRY(d, hipMemset(d->w.stamps, 0, NBL_STAMP_SLOTS * 8));
	if (!on) d->w.stamps = nullptr;
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): 0 = every decode runs the check-node pass of its last iteration itself, 1 (the
// default) = undamped fused EMS leaves it to the first reader of the message state (finish_pending).  Tests and A/B runs compare both.
extern "C" nbl_status nbl_debug_defer_last(nbl_decoder *d, int32_t on)
{
	if (!d) return NBL_ERR_ARG;
	d->defer_last = on != 0;
	return NBL_OK;
}

extern "C" nbl_status nbl_set_record_state(nbl_decoder *d, int32_t on)
{
	if (!d) return NBL_ERR_ARG;
	d->record_state = on != 0;
	return NBL_OK;
}

extern "C" nbl_status nbl_last_timing(nbl_decoder *d, double ms[4], int64_t launches[3])
{
	if (!d) return NBL_ERR_ARG;
	if (ms) memcpy(ms, d->ms, sizeof d->ms);
	if (launches) for (int i = 0; i < 3; i++) launches[i] = d->launches[i];
	// A check-node pass the decode left pending (finish_pending): a profiled call counts the launches its times cover, so that
	// ms[2] / launches[2] stays the time of one launch -- the pass is counted when it runs.  Without profiling the counters describe
	// the call's schedule, one check-node pass per iteration, run by now or owed.
	if (launches && d->pending.on && !d->pending.timed) launches[2]++;
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): the kernel choice for a code description -- the shape and the plan, nothing else;
// no device, no decoder, no field tables.
struct nbl_plan_info { const char *cn; int32_t fusable, fused, want_v2c; };
static nbl_status plan_info(const nbl_code_desc *code, const nbl_params *params, NblKind kind, bool layered, int32_t force_generic, int32_t record_state,
                            nbl_plan_info *out)
{
	if (!code || !params || !out || code->N <= 0 || code->M <= 0) return NBL_ERR_ARG;
	const NblPlan plan = nbl_plan(nbl_shape(code), *params, NblPlanReq{kind, layered, force_generic, record_state != 0, small_enabled()});
	*out = {nbl_plan_name(plan), plan.fusable, plan.fused, plan.want_v2c};
	return NBL_OK;
}

// The decoder nbl_create* / nbl_create_layered* would make.  layered_flags: NBL_LAYERED_* of nbl_create_layered_ex, -1 = the flooding
// schedule; ext: as nbl_create_ex takes it (the plan reads nothing of it)
extern "C" nbl_status nbl_debug_plan(const nbl_code_desc *code, const nbl_params *params, const nbl_params_ext *, int32_t layered_flags,
                                     int32_t force_generic, int32_t record_state, nbl_plan_info *out)
{
	return plan_info(code, params, NBL_KIND_BASE, layered_flags >= 0, force_generic, record_state, out);
}

// The decoder the entry point of a kind would make.  kind_name: "fht", "fht32", "fht32_wide", "ems_wide", "tems_wide", "bp_wide" or "minmax" (NblEntry::name);
// layered: nonzero = with the kind's NBL_*_LAYERED flag
extern "C" nbl_status nbl_debug_plan_kind(const nbl_code_desc *code, const nbl_params *params, const char *kind_name, int32_t layered,
                                          int32_t force_generic, int32_t record_state, nbl_plan_info *out)
{
	const NblEntry *en = nbl_entry_named(kind_name);
	return en ? plan_info(code, params, en->kind, layered != 0, force_generic, record_state, out) : NBL_ERR_ARG;
}

// Diagnostic only (not part of include/nbldpc.h): the bytes of LDS one check of an nbl_create_ems_wide decoder takes -- the one function
// creation's refusal and both launchers use
extern "C" uint64_t nbl_debug_ems_wide_lds_bytes(int32_t q, int32_t maxdc, int32_t nm, int32_t nc) { return nbl_ems_wide_lds_bytes(q, maxdc, nm, nc); }

// Diagnostic only (not part of include/nbldpc.h): the bytes of LDS one check of the wide T-EMS programme takes -- the one function
// creation's refusal and both launchers use
extern "C" uint64_t nbl_debug_tems_wide_lds_bytes(int32_t q, int32_t maxdc, int32_t nr, int32_t nc) { return nbl_tems_wide_lds_bytes(q, maxdc, nr, nc); }

// Diagnostic only (not part of include/nbldpc.h): the bytes of LDS one check of the wide log-QSPA programme takes -- the one function both
// launchers size by (below 160 KB for every shape the ABI accepts: creation has nothing to refuse)
extern "C" uint64_t nbl_debug_bp_wide_lds_bytes(int32_t q, int32_t maxdc) { return nbl_bp_wide_lds_bytes(q, maxdc); }

// Diagnostic only (not part of include/nbldpc.h): the bytes of LDS one check of an nbl_create_minmax decoder takes -- the one function both
// launchers size by, and the figure include/nbldpc.h quotes
extern "C" uint64_t nbl_debug_minmax_lds_bytes(int32_t q, int32_t maxdc) { return nbl_minmax_lds_bytes(q, maxdc); }

// Diagnostic only (not part of include/nbldpc.h): the path code (nbl_tems_path.h) of the path that deviates to syms[i] in column cols[i],
// i < n <= NBL_TEMS_WIDE_MAX_NC, columns ascending -- built by the kernels' own append, one deviation after the other; 0 for arguments
// outside that
extern "C" uint64_t nbl_debug_tems_wide_path_key(const int32_t *cols, const int32_t *syms, int32_t n)
{
	if (n < 0 || n > NBL_TEMS_WIDE_MAX_NC || (n > 0 && (!cols || !syms))) return 0;
	uint64_t code = 0;
	for (int i = 0; i < n; i++) {
		if (cols[i] < 0 || cols[i] > 31 || syms[i] < 1 || syms[i] > 255 || (i > 0 && cols[i] <= cols[i - 1])) return 0;
		code = nbl_tems_path_append(code, i + 1, cols[i], syms[i]);
	}
	return code;
}

// Diagnostic only: the digit of column `col` of a path code, by the kernels' own extraction
extern "C" int32_t nbl_debug_tems_wide_path_digit(uint64_t code, int32_t col) { return (col < 0 || col > 31) ? -1 : nbl_tems_path_digit(code, col); }

struct LayerRange { int off, cnt; }; // checks ly.chk[off .. off + cnt) : one layer

static bool cn_is_layered(NblCn cn)
{
	switch (cn) {
	case NBL_CN_EMS_LAYERED: case NBL_CN_TEMS_LAYERED: case NBL_CN_BP_LAYERED: case NBL_CN_FHT_LAYERED: case NBL_CN_EMS_WIDE_LAYERED:
	case NBL_CN_TEMS_WIDE_LAYERED: case NBL_CN_BP_WIDE_LAYERED: case NBL_CN_FHT_WIDE_LAYERED: return true;
	default: return false;
	}
}

// The one launch of check-node kernel `cn`; fused: with the variable-node pass inside (w then carries c2v_prev).  The layered kernels
// run once per layer: `lr` names the layer's checks, and is NULL for every other kernel.
static nbl_status launch_cn(nbl_decoder *d, NblCn cn, const NblWork &w, const NblRun &r, bool fused, hipStream_t st, const LayerRange *lr = nullptr)
{
	const NblGraphDev &g = d->g;
	const bool f32 = nbl_kind_f32(d->kind); // (NblPlan::f32: the FHT kinds run by their binary32 instances on the float state)
	const bool mm = d->kind == NBL_KIND_MINMAX; // (NblPlan::minmax: the launch shape of the wide EMS kinds, run by the Min-Max programme)
	if (cn_is_layered(cn) != (lr != nullptr)) { d->err = "layered schedule: no layered check-node kernel for this method"; return NBL_ERR_UNSUPPORTED; }
	const int off = lr ? lr->off : 0, cnt = lr ? lr->cnt : 0;
	switch (cn) {
	case NBL_CN_EMS256: HIP_TRY(d, nbl_launch_cn_ems256(g, w, r, fused, st)); break;
	case NBL_CN_EMS_SMALL: HIP_TRY(d, nbl_launch_cn_ems_small(g, w, r, fused, st)); break;
	case NBL_CN_EMS64: HIP_TRY(d, nbl_launch_cn_ems64(g, w, r, fused, st)); break;
	case NBL_CN_EMS: HIP_TRY(d, nbl_launch_cn_ems(g, w, r, st)); break;
	case NBL_CN_TEMS64: HIP_TRY(d, nbl_launch_cn_tems64(g, w, r, fused, st)); break;
	case NBL_CN_TEMS256: HIP_TRY(d, nbl_launch_cn_tems256(g, w, r, fused, st)); break;
	case NBL_CN_TEMS_SMALL: HIP_TRY(d, nbl_launch_cn_tems_small(g, w, r, fused, st)); break;
	case NBL_CN_TEMS: HIP_TRY(d, nbl_launch_cn_tems(g, w, r, st)); break;
	case NBL_CN_BP256: HIP_TRY(d, nbl_launch_cn_bp256(g, w, r, fused, st)); break;
	case NBL_CN_BP64: HIP_TRY(d, nbl_launch_cn_bp64(g, w, r, fused, st)); break;
	case NBL_CN_BP_SMALL: HIP_TRY(d, nbl_launch_cn_bp_small(g, w, r, fused, st)); break;
	case NBL_CN_BP: HIP_TRY(d, nbl_launch_cn_bp(g, w, r, st)); break;
	case NBL_CN_FHT: HIP_TRY(d, f32 ? nbl_launch_cn_fht32(g, w, d->w32, r, st) : nbl_launch_cn_fht(g, w, r, st)); break;
	case NBL_CN_FHT_WIDE: HIP_TRY(d, f32 ? nbl_launch_cn_fht32_wide(g, w, d->w32, r, st) : nbl_launch_cn_fht_wide(g, w, r, st)); break;
	case NBL_CN_EMS_WIDE: HIP_TRY(d, mm ? nbl_launch_cn_minmax(g, w, r, st) : nbl_launch_cn_ems_wide(g, w, r, st)); break;
	case NBL_CN_TEMS_WIDE: HIP_TRY(d, nbl_launch_cn_tems_wide(g, w, r, st)); break;
	case NBL_CN_BP_WIDE: HIP_TRY(d, nbl_launch_cn_bp_wide(g, w, r, st)); break;
	case NBL_CN_BSTEMS: HIP_TRY(d, nbl_launch_cn_bstems(g, w, r, st)); break;
	case NBL_CN_EMS_LAYERED: HIP_TRY(d, nbl_launch_cn_ems_layered(g, w, r, d->ly, off, cnt, st)); break;
	case NBL_CN_TEMS_LAYERED: HIP_TRY(d, nbl_launch_cn_tems_layered(g, w, r, d->ly, off, cnt, st)); break;
	case NBL_CN_BP_LAYERED: HIP_TRY(d, nbl_launch_cn_bp_layered(g, w, r, d->ly, off, cnt, st)); break;
	case NBL_CN_FHT_LAYERED:
		HIP_TRY(d, f32 ? nbl_launch_cn_fht32_layered(g, w, d->w32, r, d->ly, off, cnt, st) : nbl_launch_cn_fht_layered(g, w, r, d->ly, off, cnt, st));
		break;
	case NBL_CN_EMS_WIDE_LAYERED:
		HIP_TRY(d, mm ? nbl_launch_cn_minmax_layered(g, w, r, d->ly, off, cnt, st) : nbl_launch_cn_ems_wide_layered(g, w, r, d->ly, off, cnt, st));
		break;
	case NBL_CN_TEMS_WIDE_LAYERED: HIP_TRY(d, nbl_launch_cn_tems_wide_layered(g, w, r, d->ly, off, cnt, st)); break;
	case NBL_CN_BP_WIDE_LAYERED: HIP_TRY(d, nbl_launch_cn_bp_wide_layered(g, w, r, d->ly, off, cnt, st)); break;
	case NBL_CN_FHT_WIDE_LAYERED:
		HIP_TRY(d, f32 ? nbl_launch_cn_fht32_wide_layered(g, w, d->w32, r, d->ly, off, cnt, st) : nbl_launch_cn_fht_wide_layered(g, w, r, d->ly, off, cnt, st));
		break;
	default: d->err = "check-node kernel for this method is not built yet"; return NBL_ERR_UNSUPPORTED;
	}
	return NBL_OK;
}

// The iteration loop of Decoding_BP / _EMS / _TEMS (NBLDPC.cpp:673 / 805 / 973): per iteration one fused launch + syndrome
// (specialised (2,4)-regular shapes) or the launch triple VN, syndrome, CN.  The launches of a window of iterations are captured
// into a hipGraph once and replayed (a decode is 100+ back-to-back launches: at small batches the gaps between them are most
// of the time).
struct IterCtx {
	nbl_decoder *d;
	NblPlan plan;
	NblRun r;
	bool damp;
	double *bufA, *bufB;
	const double *zeros = nullptr; // stands in for bufA in iteration 1 (then bufA needs no clearing)
	int batch = 0;                 // codewords of the call (r.B may shrink to the active list; the OSD sums cover every codeword)
	bool defer = false;            // iteration max_iter runs its variable-node half alone (defers_last)
	// profiling: one event after every launch on the launch stream; phase time = sum of the gaps it closes
	size_t nev = 0;
	std::vector<int> tag; // 0 vn, 1 syn, 2 cn, 3 other
};

static hipError_t mark(IterCtx &c, int t, hipStream_t st)
{
	nbl_decoder *d = c.d;
	if (!d->profiling) return hipSuccess;
	if (c.nev == d->pev.size()) { hipEvent_t e; hipError_t rc = hipEventCreate(&e); if (rc != hipSuccess) return rc; d->pev.push_back(e); }
	c.tag.push_back(t);
	return hipEventRecord(d->pev[c.nev++], st);
}

// Whether the decode leaves the check-node half of iteration max_iter to finish_pending.  Nothing a decode returns depends on that
// pass: its c2v would be read by an iteration max_iter + 1 that never runs.  Undamped fused EMS only -- the damped fused kernels keep
// per-edge decision and v2c state in their variable-node stage -- and only while nothing records or accumulates per iteration.
static bool defers_last(const nbl_decoder *d, const NblPlan &plan)
{
	return d->defer_last && plan.fused && d->prm.method == NBL_METHOD_EMS && d->prm.max_iter >= 2 && !d->layered && !d->record_state &&
	       !d->osd_acc && !d->osd_on && !d->w.post && !d->w.stamps;
}

// The variable-node pass of the flooding schedule (v2c, posterior, decision), and that of the layered one (posterior and decision from
// the c2v as it stands); on a binary32 plan the same passes on the float state, the flooding one damped
static hipError_t launch_vn(const IterCtx &c, hipStream_t st)
{
	const nbl_decoder *d = c.d;
	return c.plan.f32 ? nbl_launch_vn32(d->g, d->w, d->w32, c.r, true, st) : nbl_launch_vn(d->g, d->w, c.r, c.damp, st);
}

static hipError_t launch_vn_decide(const IterCtx &c, hipStream_t st)
{
	const nbl_decoder *d = c.d;
	return c.plan.f32 ? nbl_launch_vn32(d->g, d->w, d->w32, c.r, false, st) : nbl_launch_vn_decide(d->g, d->w, c.r, st);
}

// launches of iterations it_lo .. it_hi on `st`
static nbl_status enqueue_window(IterCtx &c, int it_lo, int it_hi, hipStream_t st, bool count)
{
	nbl_decoder *d = c.d;
	for (int it = it_lo; it <= it_hi; it++) {
		c.r.iter = it;
		if (d->layered) {
			// decision and syndrome from the c2v the previous iteration left, then the layers in order, each on the c2v the layers
			// before it have just written (one buffer; the launches of a stream run in order)
			HIP_TRY(d, launch_vn_decide(c, st));
			HIP_TRY(d, mark(c, 0, st));
			HIP_TRY(d, nbl_launch_syn(d->g, d->w, c.r, st));
			HIP_TRY(d, mark(c, 1, st));
			// (T-EMS, log-QSPA: each check also damps its inputs against the v2c buffer and updates it in place; init_kernel has set
			// v2c = L_ch)
			for (int l = 0; l < d->n_layers; l++) {
				const LayerRange lr = {d->h_lay_off[l], d->h_lay_off[l + 1] - d->h_lay_off[l]};
				if (const nbl_status s = launch_cn(d, c.plan.cn, d->w, c.r, false, st, &lr)) return s;
			}
			HIP_TRY(d, mark(c, 2, st));
			if (count) { d->launches[0]++; d->launches[1]++; d->launches[2] += d->n_layers; }
			continue;
		}
		if (c.plan.fused && c.defer && it == d->prm.max_iter) {
			// the last iteration: posterior and decision from the c2v of iteration max_iter - 1 (the layered schedule's pass: the same
			// sums in the same order, the same decision rule), then the syndrome.  Tagged "other": no time is variable-node time on
			// the fused path.
			NblWork wv = d->w;
			wv.c2v = (it & 1) ? c.bufA : c.bufB;
			HIP_TRY(d, nbl_launch_vn_decide(d->g, wv, c.r, st));
			HIP_TRY(d, mark(c, 3, st));
			HIP_TRY(d, nbl_launch_syn(d->g, d->w, c.r, st));
			HIP_TRY(d, mark(c, 1, st));
			if (count) d->launches[1]++;
			continue;
		}
		if (c.plan.fused) {
			// one launch = variable-node pass + check-node pass; c2v ping-pongs between the two buffers
			NblWork wf = d->w;
			wf.c2v_prev = (it == 1 && c.zeros) ? c.zeros : (it & 1) ? c.bufA : c.bufB;
			wf.c2v_prev_shared = (it == 1 && c.zeros) ? 1 : 0;
			wf.c2v = (it & 1) ? c.bufB : c.bufA;
			wf.store_v2c = d->record_state ? 1 : 0;
			const nbl_status s = launch_cn(d, c.plan.cn, wf, c.r, true, st);
			if (s) return s;
			HIP_TRY(d, mark(c, 2, st));
			if (d->osd_acc) {
				HIP_TRY(d, nbl_launch_osd_acc(d->w.post, d->ws.osd_S, c.batch, d->g.N, d->g.p, d->g.q, d->osd_factor, it == 1, st));
				HIP_TRY(d, mark(c, 3, st));
			}
			HIP_TRY(d, nbl_launch_syn(d->g, d->w, c.r, st));
			HIP_TRY(d, mark(c, 1, st));
			if (count) { d->launches[2]++; d->launches[1]++; }
			continue;
		}
		HIP_TRY(d, launch_vn(c, st));
		HIP_TRY(d, mark(c, 0, st));
		if (d->osd_acc) {
			HIP_TRY(d, nbl_launch_osd_acc(d->w.post, d->ws.osd_S, c.batch, d->g.N, d->g.p, d->g.q, d->osd_factor, it == 1, st));
			HIP_TRY(d, mark(c, 3, st));
		}
		HIP_TRY(d, nbl_launch_syn(d->g, d->w, c.r, st));
		HIP_TRY(d, mark(c, 1, st));
		if (count) { d->launches[0]++; d->launches[1]++; }
		// (the reference leaves the loop after the syndrome check of the last iteration it runs; the check-node pass of a
		// window's last iteration is only needed if another window follows.  It is not cheap -- one check-node launch per call --
		// and the fused EMS path above defers it; here c2v is updated in place and nbl_read_state returns it, so it stays)
		const nbl_status s = launch_cn(d, c.plan.cn, d->w, c.r, false, st);
		if (s) return s;
		HIP_TRY(d, mark(c, 2, st));
		if (count) d->launches[2]++;
	}
	return NBL_OK;
}

// Run window number `widx` (iterations it_lo..it_hi): replay its graph, capturing it first if needed; plain launches when
// graphs are off, while profiling (events between the launches) or if the capture fails.
static nbl_status run_window(IterCtx &c, int widx, int it_lo, int it_hi, hipStream_t st)
{
	nbl_decoder *d = c.d;
	const bool graph_ok = d->use_graph && !d->profiling && !d->w.stamps;
	if (graph_ok) {
		if ((int)d->gexec.size() <= widx) d->gexec.resize(widx + 1, nullptr);
		if (!d->gexec[widx]) {
			hipGraph_t graph = nullptr;
			if (hipStreamBeginCapture(d->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
				const nbl_status s = enqueue_window(c, it_lo, it_hi, d->stream, false);
				const hipError_t e = hipStreamEndCapture(d->stream, &graph);
				if (s == NBL_OK && e == hipSuccess && graph) {
					if (hipGraphInstantiate(&d->gexec[widx], graph, nullptr, nullptr, 0) != hipSuccess) d->gexec[widx] = nullptr;
				}
				if (graph) (void)hipGraphDestroy(graph);
				(void)hipGetLastError();
			}
			if (!d->gexec[widx]) d->use_graph = false; // capture is not available here: plain launches from now on
		}
		if (d->gexec[widx]) {
			HIP_TRY(d, hipGraphLaunch(d->gexec[widx], st));
			const int n = it_hi - it_lo + 1;
			d->launches[1] += n; d->launches[2] += d->layered ? (long long)n * d->n_layers : n;
			if (c.defer && it_hi == d->prm.max_iter) d->launches[2]--; // (the captured window holds the deferred form)
			if (!c.plan.fused) d->launches[0] += n;
			return NBL_OK;
		}
	}
	return enqueue_window(c, it_lo, it_hi, st, true);
}

nbl_status run_iterations(nbl_decoder *d, const double *d_Lin, int B, hipStream_t st)
{
	const nbl_params &p = d->prm;
	IterCtx c;
	c.d = d;
	d->pending.on = false; // (a pass the last decode left pending is dropped: nobody read that state)
	d->idd_sub = false; // (the loop sets it again after its last pass)
	const bool as_ems = p.method == NBL_METHOD_EMS || d->kind == NBL_KIND_MINMAX; // (Min-Max: the EMS iteration around its own check node)
	c.damp = !as_ems;
	NblRun &r = c.r;
	r = NblRun{};
	r.B = B;
	r.fixed_iters = p.fixed_iters;
	if (as_ems) { r.nm = p.ems_nm; r.nc = p.ems_nc; r.factor = p.ems_factor; r.offset = p.ems_offset; }
	else if (p.method == NBL_METHOD_BS_TEMS) { r.nm = d->ext.bs_nm; r.nc = d->ext.bs_nc; r.factor = d->ext.bs_factor; r.offset = d->ext.bs_offset; }
	else { r.nr = p.tems_nr; r.nc = p.tems_nc; r.factor = p.tems_factor; r.offset = p.tems_offset; }
	r.damp_old = (p.method == NBL_METHOD_BP) ? 0.5 : 0.25;  // NBLDPC.cpp:739 / :1046 / :1262
	r.damp_new = (p.method == NBL_METHOD_BP) ? 0.5 : 0.75;
	d->launches[0] = d->launches[1] = d->launches[2] = 0;
	c.plan = plan_of(d); // (ensure_workspace has made c2v_alt and c2v_zero for every fusable shape)
	c.bufA = d->w.c2v;
	c.bufB = d->ws.c2v_alt;
	c.zeros = c.plan.fused ? d->ws.c2v_zero.p : nullptr;
	c.defer = defers_last(d, c.plan);
	// the captured graphs hold buffer addresses and the batch size: any change drops them
	const nbl_decoder::GraphKey key = {d_Lin, d->w.Lch, d->w.v2c, d->w.c2v, d->ws.c2v_alt, d->w.post, d->ws.osd_S, B, d->record_state ? 1 : 0, d->force_generic, c.plan.fused ? (c.defer ? 3 : 1) : 0};
	c.batch = B;
	if (memcmp(&key, &d->gkey, sizeof key) != 0) { drop_graphs(d); d->gkey = key; }
	HIP_TRY(d, mark(c, 3, st));
	// (nbl_create_fht32: L_ch and the flags alone -- no FP64 message buffer need exist; then the one narrowing launch of the call, which
	// also sets the float v2c = Lf and c2v = 0.  Its time is in ms[3] alone: nbl_last_timing has no launch counter for it)
	HIP_TRY(d, nbl_launch_init(d_Lin, d->g, d->w, B, c.plan.f32 ? 2 : (c.damp ? 1 : 0) | (c.zeros ? 2 : 0), st)); // bit 1: c2v is not cleared
	HIP_TRY(d, mark(c, 3, st));
	if (c.plan.f32) {
		HIP_TRY(d, nbl_launch_narrow32(d->g, d->w.Lch, d->w32, B, st));
		HIP_TRY(d, mark(c, 3, st));
		d->wide_valid = false;
	}
	d->last_c2v = c.zeros ? c.zeros : c.bufA;
	d->last_fused = c.plan.fused;
	// windows: fixed iterations or no polling -> one window; early exit -> `poll_every` iterations, then ask the device
	const bool polling = !p.fixed_iters && p.poll_every > 0;
	const int wlen = polling ? p.poll_every : (p.max_iter > 0 ? p.max_iter : 1);
	int last_it = 0;
	if (polling && d->h_ndone.grow(d->err, 2 * sizeof(int))) return NBL_ERR_HIP;
	// Early exit without idling the GPU: window w+1 is queued BEFORE the host looks at the count of converged codewords that
	// window w left behind (read back through pinned memory behind an event).  If everything had converged, the extra window
	// finds every codeword frozen and its kernels return at once; outputs, flags and iteration counts are unaffected.
	// Large batches: after every window the device rebuilds the list of codewords still iterating, and the grids of the next
	// windows cover that list -- sized by the newest converged count the host has seen, an upper bound of the list's length --
	// instead of the whole batch (most codewords of a waterfall batch are done long before the stragglers).
	const bool compact = polling && d->use_compact && !d->use_graph && B >= 1024;
	d->w.active = nullptr;
	int pending = -1; // parity of the read-back that has not been looked at yet
	const int max_iter = p.method == NBL_METHOD_OSD ? 0 : p.max_iter; // (method 6: Decoding_OSD_bit alone, no iterations)
	for (int it_lo = 1, widx = 0; it_lo <= max_iter; it_lo += wlen, widx++) {
		const int it_hi = (it_lo + wlen - 1 < p.max_iter) ? it_lo + wlen - 1 : p.max_iter;
		nbl_status s = run_window(c, widx, it_lo, it_hi, st);
		if (s) { d->w.active = nullptr; return s; }
		last_it = it_hi;
		if (polling) {
			const int par = widx & 1;
			HIP_TRY(d, hipMemcpyAsync(&d->h_ndone[par], d->w.n_done, sizeof(int), hipMemcpyDeviceToHost, st));
			HIP_TRY(d, hipEventRecord(d->ev[par], st));
			if (compact) {
				HIP_TRY(d, nbl_launch_compact(d->w.done, B, d->ws.active, (int *)d->w.n_act, st));
				d->w.active = d->ws.active;
			}
			if (pending >= 0) {
				HIP_TRY(d, hipEventSynchronize(d->ev[pending]));
				if (d->h_ndone[pending] >= B) break;
				if (compact) c.r.B = B - d->h_ndone[pending];
			}
			pending = par;
		}
	}
	d->w.active = nullptr;
	// OSD on every codeword that did not converge (NBLDPC.cpp:769-775: only after at least one iteration), or the whole of method 6
	if (d->osd_on && (p.method == NBL_METHOD_OSD || p.max_iter > 0)) {
		NblOsdDev o = d->osd;
		o.S = d->ws.osd_S;
		HIP_TRY(d, nbl_launch_osd(d->g, d->w, o, B, st));
		HIP_TRY(d, mark(c, 3, st));
	}
	if (polling) HIP_TRY(d, hipStreamSynchronize(st));
	if (c.plan.fused && last_it > 0) d->last_c2v = (last_it & 1) ? c.bufB : c.bufA;
	if (c.defer && last_it == p.max_iter) {
		// iteration max_iter ran without its check-node half: until finish_pending the last c2v is that of iteration max_iter - 1.
		// The late launch covers the whole batch: under early exit it returns at once for every codeword that is done by now.
		nbl_decoder::Pending &pd = d->pending;
		pd.iter = last_it;
		pd.prev = (last_it & 1) ? c.bufA : c.bufB;
		pd.out = (last_it & 1) ? c.bufB : c.bufA;
		pd.batch = B;
		pd.cn = c.plan.cn;
		pd.r = c.r;
		pd.r.iter = last_it;
		pd.r.B = B;
		pd.timed = d->profiling;
		pd.foreign = st != d->stream;
		if (pd.foreign) {
			if (!d->pending_ev) HIP_TRY(d, hipEventCreateWithFlags(&d->pending_ev, hipEventDisableTiming));
			HIP_TRY(d, hipEventRecord(d->pending_ev, st));
		}
		d->last_c2v = pd.prev;
		pd.on = true;
	}
	if (d->profiling && c.nev > 0) {
		HIP_TRY(d, hipEventSynchronize(d->pev[c.nev - 1]));
		d->ms[0] = d->ms[1] = d->ms[2] = d->ms[3] = 0;
		for (size_t i = 1; i < c.nev; i++) {
			float ms = 0;
			HIP_TRY(d, hipEventElapsedTime(&ms, d->pev[i - 1], d->pev[i]));
			if (c.tag[i] < 3) d->ms[c.tag[i]] += ms;
			d->ms[3] += ms;
		}
	}
	d->last_B = B;
	return NBL_OK;
}

nbl_status finish_pending(nbl_decoder *d, hipStream_t reader)
{
	nbl_decoder::Pending &pd = d->pending;
	if (!pd.on) return NBL_OK;
	// exactly the fused launch the decode skipped: L_ch and the c2v of iteration max_iter - 1 are intact until the next decode, and the
	// launch rewrites dec with the values the variable-node pass left there
	if (pd.foreign) HIP_TRY(d, hipStreamWaitEvent(d->stream, d->pending_ev, 0));
	NblWork wf = d->w;
	wf.active = nullptr;
	wf.c2v_prev = pd.prev;
	wf.c2v_prev_shared = 0;
	wf.c2v = pd.out;
	wf.store_v2c = 0;
	if (const nbl_status s = launch_cn(d, pd.cn, wf, pd.r, true, d->stream)) return s;
	d->last_c2v = pd.out;
	d->launches[2]++; // (with pd.on cleared below nbl_last_timing stops adding the owed pass: the count moves only for a profiled call)
	pd.on = false;
	if (reader && reader != d->stream) {
		if (!d->pending_ev) HIP_TRY(d, hipEventCreateWithFlags(&d->pending_ev, hipEventDisableTiming));
		HIP_TRY(d, hipEventRecord(d->pending_ev, d->stream));
		HIP_TRY(d, hipStreamWaitEvent(reader, d->pending_ev, 0));
	}
	return NBL_OK;
}

nbl_status read_back(nbl_decoder *d, const int *out, const uint8_t *done, const int *iters, int B, int32_t *to_out, uint8_t *to_done,
                     int32_t *to_iters, hipMemcpyKind kind, hipStream_t st, bool sync)
{
	HIP_TRY(d, hipMemcpyAsync(to_out, out, (size_t)B * d->g.N * 4, kind, st));
	if (to_done) HIP_TRY(d, hipMemcpyAsync(to_done, done, (size_t)B, kind, st));
	if (to_iters) HIP_TRY(d, hipMemcpyAsync(to_iters, iters, (size_t)B * 4, kind, st));
	if (sync) HIP_TRY(d, hipStreamSynchronize(st));
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_device(nbl_decoder *d, const double *d_L_ch, int32_t B, int32_t *d_out_sym,
                                              uint8_t *d_converged, int32_t *d_iters, void *stream)
{
	if (!d || !d_L_ch || !d_out_sym || B < 0) return NBL_ERR_ARG;
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	hipStream_t st = stream ? (hipStream_t)stream : d->stream;
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	if ((s = run_iterations(d, d_L_ch, B, st))) return s;
	return read_back(d, d->w.out, d->w.done, d->w.iters, B, d_out_sym, d_converged, d_iters, hipMemcpyDeviceToDevice, st, false);
}

extern "C" nbl_status nbl_decode_batch(nbl_decoder *d, const double *L_ch, int32_t B, int32_t *out_sym, uint8_t *converged,
                                       int32_t *iters)
{
	if (!d || !L_ch || !out_sym || B < 0) return NBL_ERR_ARG;
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	const size_t in_bytes = (size_t)B * d->g.N * (d->g.q - 1) * 8;
	if ((s = d->ws.Lin.grow(d->err, (size_t)d->cap * d->g.N * (d->g.q - 1) * 8))) return s; // (made once per workspace: cap only moves with it)
	HIP_TRY(d, hipMemcpyAsync(d->ws.Lin, L_ch, in_bytes, hipMemcpyHostToDevice, d->stream));
	if ((s = run_iterations(d, d->ws.Lin, B, d->stream))) return s;
	return read_back(d, d->w.out, d->w.done, d->w.iters, B, out_sym, converged, iters, hipMemcpyDeviceToHost, d->stream, true);
}

// Diagnostic only (not part of include/nbldpc.h): the batch size of the last decode call -- what nbl_soft_output's buffers are sized by
extern "C" int32_t nbl_debug_last_batch(const nbl_decoder *d) { return d ? d->last_B : 0; }

// Diagnostic only: channel LLRs of codeword b as the decoder holds them, [N][q-1]
extern "C" nbl_status nbl_debug_read_lch(nbl_decoder *d, int32_t b, double *out)
{
	if (!d || !out || b < 0 || b >= d->last_B) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	const int q = d->g.q, N = d->g.N;
	DevBuf<double> tmp;
	if (nbl_status s = tmp.grow(d->err, (size_t)N * (q - 1) * 8)) return s;
	HIP_TRY(d, nbl_launch_unpad(d->w.Lch + (size_t)b * N * q, tmp, nullptr, N, q, d->stream));
	HIP_TRY(d, hipMemcpyAsync(out, tmp, (size_t)N * (q - 1) * 8, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

extern "C" nbl_status nbl_read_state(nbl_decoder *d, int32_t b, double *post, double *v2c, double *c2v)
{
	if (!d) return NBL_ERR_ARG;
	if (d->idd_sub) { d->err = std::string("nbl_read_state") + NBL_IDD_SUB_TEXT; return NBL_ERR_ARG; }
	if (b < 0 || b >= d->last_B) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	const int q = d->g.q, N = d->g.N, E = d->g.E;
	if (nbl_status s = widen_state(d)) return s; // (nbl_create_fht32: the doubles below are the exact widening of the float state)
	DevBuf<double> tmp;
	if (nbl_status s = tmp.grow(d->err, (size_t)E * (q - 1) * 8)) return s;
	nbl_status rc = NBL_OK;
	auto grab = [&](const double *src, const int *map, int rows, double *dst) -> nbl_status {
		HIP_TRY(d, nbl_launch_unpad(src, tmp, map, rows, q, d->stream));
		HIP_TRY(d, hipMemcpyAsync(dst, tmp, (size_t)rows * (q - 1) * 8, hipMemcpyDeviceToHost, d->stream));
		HIP_TRY(d, hipStreamSynchronize(d->stream));
		return NBL_OK;
	};
	if (post) {
		if (!d->w.post) { d->err = "state recording was off during the last decode (nbl_set_record_state)"; rc = NBL_ERR_ARG; }
		else rc = grab(d->w.post + (size_t)b * N * q, nullptr, N, post);
	}
	if (!rc && v2c) {
		if (d->kind == NBL_KIND_MINMAX) { d->err = "a Min-Max decoder returns no v2c (as the EMS decoders: post and c2v are its state)"; rc = NBL_ERR_UNSUPPORTED; }
		else if (d->layered && d->prm.method == NBL_METHOD_EMS) { d->err = "the layered schedule never materialises v2c (a check forms its inputs from L_ch and c2v)"; rc = NBL_ERR_UNSUPPORTED; }
		else if (!d->w.v2c) { d->err = "v2c is not kept in HBM on the fused path unless state recording is on (nbl_set_record_state)"; rc = NBL_ERR_ARG; }
		else rc = grab(d->w.v2c + (size_t)b * E * q, nullptr, E, v2c);
	}
	if (!rc && c2v) rc = finish_pending(d);
	if (!rc && c2v) {
		const double *src = d->last_c2v ? d->last_c2v : d->w.c2v;
		if (d->last_fused && d->ws.c2v_alt && !d->prm.fixed_iters) {
			// fused iterations: a codeword that converged at iteration k has c2v(k) in one buffer (computed before its syndrome was
			// known) and c2v(k-1), what the reference returns with, intact in the other; iteration i writes bufB when i is odd
			int it = 0;
			uint8_t done = 0;
			HIP_TRY(d, hipMemcpy(&it, d->w.iters + b, sizeof it, hipMemcpyDeviceToHost));
			HIP_TRY(d, hipMemcpy(&done, d->w.done + b, 1, hipMemcpyDeviceToHost));
			if (done) src = (it == 1 && d->ws.c2v_zero) ? d->ws.c2v_zero : ((it - 1) & 1) ? d->ws.c2v_alt : d->w.c2v; // buffer written by iteration it-1 (it = 1: the zeros)
		}
		rc = grab(src == d->ws.c2v_zero ? src : src + (size_t)b * E * q, d->d_e2c_map, E, c2v); // (the zeros are one shared block)
	}
	return rc;
}

// Diagnostic only (not part of include/nbldpc.h): the flag-0 OSD posterior sums S of codeword b after the last decode, [N][p]
extern "C" nbl_status nbl_debug_osd_sums(nbl_decoder *d, int32_t b, double *out)
{
	if (!d || !out || b < 0 || b >= d->last_B) return NBL_ERR_ARG;
	if (!d->ws.osd_S) { d->err = "no OSD sums: OSD post-processing with flag 0 is off"; return NBL_ERR_ARG; }
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	const size_t n = (size_t)d->g.N * d->g.p;
	HIP_TRY(d, hipMemcpyAsync(out, d->ws.osd_S + (size_t)b * n, n * 8, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}
