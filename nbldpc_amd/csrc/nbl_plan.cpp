// nbldpc_amd/csrc/nbl_plan.cpp -- which check-node kernel runs, whether the iteration is fused, which buffers must exist.
//
// Precedence of the specialised kernels (the first that can run the shape; the general kernel otherwise):
//   EMS       256, small, 64
//   T-EMS     64, 256, small
//   log-QSPA  256, 64, small     (so a (.,4)-regular GF(64) code with variables of degree 3 runs BP-64 unfused, although BP-small
//                                 could run fused there: changing that is a performance decision, and needs a measurement)
// The fused iteration is the same kernel with the variable-node pass inside; it needs the per-edge neighbour rows the kernel reads.
#include "nbl_plan.h"
#include "nbl_tems_path.h" // NBL_TEMS_WIDE_MAX_NC

NblShape nbl_shape(const nbl_code_desc *code)
{
	NblShape s{};
	s.q = code->q;
	while ((1 << s.p) < s.q) s.p++;
	s.min_dc = code->chk_deg[0];
	s.mindv = code->var_deg[0];
	for (int m = 0; m < code->M; m++) {
		const int dc = code->chk_deg[m];
		s.maxdc = dc > s.maxdc ? dc : s.maxdc;
		s.min_dc = dc < s.min_dc ? dc : s.min_dc;
	}
	for (int n = 0; n < code->N; n++) {
		const int dv = code->var_deg[n];
		s.maxdv = dv > s.maxdv ? dv : s.maxdv;
		s.mindv = dv < s.mindv ? dv : s.mindv;
	}
	s.all_dc4 = s.min_dc == 4 && s.maxdc == 4;
	s.all_dv2 = s.mindv == 2 && s.maxdv == 2;
	return s;
}

static const char *const cn_names[NBL_CN_COUNT] = {
	"ems256", "ems_small", "ems64", "ems", "tems64", "tems256", "tems_small", "tems", "bp256", "bp64", "bp_small", "bp",
	"bstems", "ems_layered", "tems_layered", "none", "bp_layered", "fht", "fht_layered", "fht_wide", "fht_wide_layered", "ems_wide", "ems_wide_layered",
	"tems_wide", "tems_wide_layered", "bp_wide", "bp_wide_layered"};

const char *nbl_cn_name(NblCn cn) { return cn_names[cn]; }
const char *nbl_plan_name(const NblPlan &plan)
{
	if (plan.minmax) return plan.cn == NBL_CN_EMS_WIDE_LAYERED ? "minmax_layered" : "minmax";
	if (!plan.f32) return cn_names[plan.cn];
	switch (plan.cn) {
	case NBL_CN_FHT_LAYERED: return "fht32_layered";
	case NBL_CN_FHT_WIDE: return "fht32_wide";
	case NBL_CN_FHT_WIDE_LAYERED: return "fht32_wide_layered";
	default: return "fht32";
	}
}

// `fusable` -- which buffers the workspace holds -- of the default plan (the base kind, switch 0) of the same request: what a wide
// programme selected by switch 3 keeps, so that the workspace does not move with a debug switch
static bool base_fusable(const NblShape &s, const nbl_params &prm, NblPlanReq rq)
{
	rq.kind = NBL_KIND_BASE;
	rq.force_generic = 0;
	return nbl_plan(s, prm, rq).fusable;
}

NblPlan nbl_plan(const NblShape &s, const nbl_params &prm, const NblPlanReq &rq)
{
	const bool layered = rq.layered, record_state = rq.record_state, small_on = rq.small_on;
	const int force_generic = rq.force_generic;
	NblPlan pl{NBL_CN_NONE, false, false, true, false, false};
	switch (rq.kind) {
	case NBL_KIND_MINMAX:
		// one programme for every degree and field, in the launch shape of the wide EMS kinds: never fused, no debug switch moves it.
		// Flooding reads the v2c of the variable-node pass; layered forms its inputs from L_ch and c2v
		pl.cn = layered ? NBL_CN_EMS_WIDE_LAYERED : NBL_CN_EMS_WIDE;
		pl.minmax = true;
		pl.want_v2c = !layered;
		return pl;
	case NBL_KIND_FHT32_WIDE:
		// the scaled programme in the degree-independent layout: a code with a larger check than the register programme holds, or
		// switch 3 at any degree; never fused; both schedules read the float v2c.  Any other request: the plan of NBL_KIND_FHT32
		if (s.maxdc > NBL_MAXDC || force_generic == 3) {
			pl.cn = layered ? NBL_CN_FHT_WIDE_LAYERED : NBL_CN_FHT_WIDE;
			pl.f32 = true;
			return pl;
		}
		[[fallthrough]];
	case NBL_KIND_FHT32: // one general kernel per schedule: never fused; both schedules read the float v2c; no debug switch moves it
		pl.cn = layered ? NBL_CN_FHT_LAYERED : NBL_CN_FHT;
		pl.f32 = true;
		return pl;
	case NBL_KIND_BP_WIDE:
		if (s.maxdc <= NBL_MAXDC && force_generic != 3) break;
		// the workgroup-per-check programme: never fused; both schedules read v2c (flooding: the inputs; layered: the damping).  With
		// maxdc <= NBL_MAXDC (switch 3) `fusable` stays that of the decoder's default plan (switch 0)
		if (s.maxdc <= NBL_MAXDC) pl.fusable = base_fusable(s, prm, rq);
		pl.cn = layered ? NBL_CN_BP_WIDE_LAYERED : NBL_CN_BP_WIDE;
		return pl;
	case NBL_KIND_TEMS_WIDE:
		if (!nbl_tems_needs_wide(s) && !(force_generic == 3 && prm.tems_nc <= NBL_TEMS_WIDE_MAX_NC)) break;
		// the workgroup-per-check programme: never fused; both schedules read v2c (flooding: the inputs; layered: the damping).  Inside
		// nbl_create's envelope (switch 3) `fusable` stays that of the decoder's default plan
		if (!nbl_tems_needs_wide(s)) pl.fusable = base_fusable(s, prm, rq);
		pl.cn = layered ? NBL_CN_TEMS_WIDE_LAYERED : NBL_CN_TEMS_WIDE;
		return pl;
	case NBL_KIND_EMS_WIDE:
		if (s.maxdc <= NBL_MAXDC && force_generic != 3) break;
		// the workgroup-per-check programme: never fused.  Flooding reads the v2c of the variable-node pass; layered forms its inputs from
		// L_ch and c2v.  With maxdc <= NBL_MAXDC (switch 3) `fusable` stays that of the decoder's default plan (switch 0)
		if (s.maxdc <= NBL_MAXDC) pl.fusable = base_fusable(s, prm, rq);
		pl.cn = layered ? NBL_CN_EMS_WIDE_LAYERED : NBL_CN_EMS_WIDE;
		pl.want_v2c = !layered;
		return pl;
	case NBL_KIND_FHT: { // one general kernel per schedule and layout: never fused; both schedules read v2c (flooding: the inputs)
		// the register programme holds DCM = NBL_MAXDC transformed inputs per lane; a code with a larger check takes the wide one.
		// Debug switches 0, 1, 2 move nothing; 3 selects the wide programme at any degree
		const bool wide = s.maxdc > NBL_MAXDC || force_generic == 3;
		pl.cn = wide ? (layered ? NBL_CN_FHT_WIDE_LAYERED : NBL_CN_FHT_WIDE) : (layered ? NBL_CN_FHT_LAYERED : NBL_CN_FHT);
		return pl;
	}
	case NBL_KIND_BASE: break;
	}
	// the base kind, and a wide kind on a code inside nbl_create's envelope
	if (layered) { // one c2v buffer updated in place: never fused; T-EMS and log-QSPA keep the v2c their damping reads
		pl.cn = prm.method == NBL_METHOD_TEMS ? NBL_CN_TEMS_LAYERED : prm.method == NBL_METHOD_BP ? NBL_CN_BP_LAYERED : NBL_CN_EMS_LAYERED;
		pl.want_v2c = prm.method == NBL_METHOD_TEMS || prm.method == NBL_METHOD_BP;
		return pl;
	}
	NblCn general = NBL_CN_NONE, special = NBL_CN_NONE;
	switch (prm.method) {
	case NBL_METHOD_EMS:
		general = NBL_CN_EMS;
		if (nbl_ems256_applicable(s, prm.ems_nm, prm.ems_nc)) special = NBL_CN_EMS256;
		else if (small_on && nbl_small_applicable(s, NBL_METHOD_EMS, prm.ems_nm, prm.ems_nc)) special = NBL_CN_EMS_SMALL;
		else if (small_on && nbl_ems64_applicable(s, prm.ems_nm, prm.ems_nc)) special = NBL_CN_EMS64;
		break;
	case NBL_METHOD_TEMS:
		general = NBL_CN_TEMS;
		if (nbl_tems64_applicable(s, prm.tems_nr, prm.tems_nc)) special = NBL_CN_TEMS64;
		else if (nbl_tems256_applicable(s, prm.tems_nr, prm.tems_nc)) special = NBL_CN_TEMS256;
		else if (small_on && nbl_small_applicable(s, NBL_METHOD_TEMS, 0, prm.tems_nc)) special = NBL_CN_TEMS_SMALL;
		break;
	case NBL_METHOD_BP:
		general = NBL_CN_BP;
		if (nbl_bp256_applicable(s)) special = NBL_CN_BP256;
		else if (nbl_bp64_applicable(s)) special = NBL_CN_BP64;
		else if (small_on && nbl_small_applicable(s, NBL_METHOD_BP, 0, 0)) special = NBL_CN_BP_SMALL;
		break;
	case NBL_METHOD_BS_TEMS: general = NBL_CN_BSTEMS; break; // (its launcher picks the field's instantiation)
	default: break;                                          // method 6: no iteration
	}
	switch (special) {
	case NBL_CN_NONE: break;
	case NBL_CN_EMS_SMALL: case NBL_CN_TEMS_SMALL: case NBL_CN_BP_SMALL: case NBL_CN_EMS64: pl.fusable = s.has_c_nbr(); break;
	default: pl.fusable = s.has_dv2_row(); break;
	}
	pl.cn = (special == NBL_CN_NONE || force_generic == 1) ? general : special;
	pl.fused = pl.fusable && force_generic == 0;
	// v2c only exists in HBM when something reads it: the unfused path, or state read-back
	// (damped methods always keep it: the damping reads the previous iteration's v2c)
	pl.want_v2c = prm.method != NBL_METHOD_EMS || !pl.fusable || record_state || force_generic != 0;
	return pl;
}
