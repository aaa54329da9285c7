// tests/plan_check.cpp -- nbl_shape() and nbl_plan() (nbldpc_amd/csrc/nbl_plan.cpp) in a stand-alone host program, for a build with
// -fsanitize=address,undefined: a handful of rows of tests/golden/cn_plan_table.json on (dv, dc)-regular shapes, with degree arrays
// that end exactly where the code description says (a read past N or M entries is an error the sanitizer reports), and rows of every
// other decoder kind, recorded from the plan queries as they stood before the kinds became one enum.
// The nbl_*_applicable predicates come from the product library.  Prints "ok <rows>"; exit status 1 on a wrong row.
#include <cstdio>
#include <cstring>
#include <vector>
#include "nbl_plan.h"

struct Row {
	NblKind kind;
	int q, dv, dc, method, nm, nc, nr, layered, force_generic, record_state, small_on;
	const char *cn; // nbl_plan_name: that of the kernel, fht32 / fht32_layered on a binary32 plan
	bool fusable, fused, want_v2c, f32;
};

static const NblKind BASE = NBL_KIND_BASE, FHT = NBL_KIND_FHT, FHT32 = NBL_KIND_FHT32, EMSW = NBL_KIND_EMS_WIDE, TEMSW = NBL_KIND_TEMS_WIDE, BPW = NBL_KIND_BP_WIDE;

static const Row rows[] = {
	// kind  q  dv dc  method             nm  nc nr lay fg rs small  kernel          fusable fused  v2c    f32
	{BASE,  256, 2, 4, NBL_METHOD_EMS,     32, 3, 0, 0, 0, 0, 1, "ems256",            true,  true,  false, false},
	{BASE,  256, 2, 4, NBL_METHOD_EMS,     32, 3, 0, 0, 1, 0, 1, "ems",               true,  false, true,  false},
	{BASE,  256, 2, 4, NBL_METHOD_EMS,     32, 3, 0, 0, 2, 0, 1, "ems256",            true,  false, true,  false},
	{BASE,  256, 2, 4, NBL_METHOD_EMS,     32, 3, 0, 0, 0, 1, 1, "ems256",            true,  true,  true,  false},
	{BASE,  256, 2, 4, NBL_METHOD_EMS,     65, 3, 0, 0, 0, 0, 1, "ems",               false, false, true,  false},
	{BASE,  256, 3, 4, NBL_METHOD_TEMS,     0, 3, 2, 0, 0, 0, 1, "tems256",           false, false, true,  false},
	{BASE,  64,  3, 4, NBL_METHOD_BP,       0, 0, 0, 0, 0, 0, 1, "bp64",              false, false, true,  false},
	{BASE,  64,  2, 6, NBL_METHOD_BP,       0, 0, 0, 0, 0, 0, 1, "bp_small",          true,  true,  true,  false},
	{BASE,  64,  2, 6, NBL_METHOD_BP,       0, 0, 0, 0, 0, 0, 0, "bp",                false, false, true,  false},
	{BASE,  64,  2, 6, NBL_METHOD_EMS,      8, 2, 0, 0, 0, 0, 1, "ems64",             true,  true,  false, false},
	{BASE,  64,  2, 6, NBL_METHOD_EMS,      8, 2, 0, 0, 0, 0, 0, "ems",               false, false, true,  false},
	{BASE,  64,  2, 4, NBL_METHOD_TEMS,     0, 3, 2, 0, 0, 0, 0, "tems64",            true,  true,  true,  false},
	{BASE,  16,  2, 4, NBL_METHOD_EMS,      8, 2, 0, 0, 0, 0, 1, "ems_small",         true,  true,  false, false},
	{BASE,  16,  4, 4, NBL_METHOD_TEMS,     0, 3, 2, 0, 0, 0, 1, "tems_small",        false, false, true,  false},
	{BASE,  16,  2, 4, NBL_METHOD_EMS,      8, 2, 0, 1, 0, 0, 1, "ems_layered",       false, false, false, false},
	{BASE,  16,  2, 4, NBL_METHOD_TEMS,     0, 3, 2, 1, 0, 0, 1, "tems_layered",      false, false, true,  false},
	{BASE,  16,  2, 4, NBL_METHOD_BS_TEMS,  4, 2, 0, 0, 0, 0, 1, "bstems",            false, false, true,  false},
	{BASE,  16,  2, 4, NBL_METHOD_OSD,      0, 0, 0, 0, 0, 0, 1, "none",              false, false, true,  false},
	{BASE,  256, 2, 4, NBL_METHOD_EMS,     32, 3, 0, 0, 3, 0, 1, "ems256",            true,  false, true,  false}, // (switch 3 is no kernel's)
	// nbl_create_fht: the register programme up to degree 8, the wide one above it or under switch 3
	{FHT,   16,  2, 4, NBL_METHOD_BP,       0, 0, 0, 0, 0, 0, 1, "fht",               false, false, true,  false},
	{FHT,   16,  2, 4, NBL_METHOD_BP,       0, 0, 0, 1, 0, 0, 1, "fht_layered",       false, false, true,  false},
	{FHT,   64,  2, 6, NBL_METHOD_BP,       0, 0, 0, 0, 2, 1, 1, "fht",               false, false, true,  false},
	{FHT,   16,  2, 4, NBL_METHOD_BP,       0, 0, 0, 0, 3, 0, 1, "fht_wide",          false, false, true,  false},
	{FHT,   16,  2, 4, NBL_METHOD_BP,       0, 0, 0, 1, 3, 0, 1, "fht_wide_layered",  false, false, true,  false},
	{FHT,   64,  2, 12, NBL_METHOD_BP,      0, 0, 0, 0, 0, 0, 1, "fht_wide",          false, false, true,  false},
	{FHT,   64,  2, 12, NBL_METHOD_BP,      0, 0, 0, 1, 1, 0, 1, "fht_wide_layered",  false, false, true,  false},
	// nbl_create_fht32: binary32 under every switch
	{FHT32, 16,  2, 4, NBL_METHOD_BP,       0, 0, 0, 0, 0, 0, 1, "fht32",             false, false, true,  true},
	{FHT32, 16,  2, 4, NBL_METHOD_BP,       0, 0, 0, 1, 0, 1, 1, "fht32_layered",     false, false, true,  true},
	{FHT32, 16,  2, 4, NBL_METHOD_BP,       0, 0, 0, 0, 3, 0, 1, "fht32",             false, false, true,  true},
	{FHT32, 64,  2, 6, NBL_METHOD_BP,       0, 0, 0, 1, 3, 0, 0, "fht32_layered",     false, false, true,  true},
	// nbl_create_ems_wide: nbl_create's plan inside its envelope; under switch 3 the wide programme with the default plan's `fusable`
	{EMSW,  16,  2, 4, NBL_METHOD_EMS,      8, 2, 0, 0, 0, 0, 1, "ems_small",         true,  true,  false, false},
	{EMSW,  16,  2, 4, NBL_METHOD_EMS,      8, 2, 0, 1, 0, 0, 1, "ems_layered",       false, false, false, false},
	{EMSW,  16,  2, 4, NBL_METHOD_EMS,      8, 2, 0, 0, 3, 0, 1, "ems_wide",          true,  false, true,  false},
	{EMSW,  16,  2, 4, NBL_METHOD_EMS,      8, 2, 0, 0, 3, 0, 0, "ems_wide",          false, false, true,  false},
	{EMSW,  16,  2, 4, NBL_METHOD_EMS,      8, 2, 0, 1, 3, 0, 1, "ems_wide_layered",  false, false, false, false},
	{EMSW,  64,  2, 12, NBL_METHOD_EMS,     8, 2, 0, 0, 0, 0, 1, "ems_wide",          false, false, true,  false},
	{EMSW,  64,  2, 12, NBL_METHOD_EMS,     8, 2, 0, 1, 2, 1, 1, "ems_wide_layered",  false, false, false, false},
	// nbl_create_tems_wide: the same; the wide programme also where the path outgrows 32 bits, and switch 3 only up to tems_nc 4
	{TEMSW, 64,  2, 4, NBL_METHOD_TEMS,     0, 3, 2, 0, 0, 0, 1, "tems64",            true,  true,  true,  false},
	{TEMSW, 64,  2, 4, NBL_METHOD_TEMS,     0, 3, 2, 1, 0, 0, 1, "tems_layered",      false, false, true,  false},
	{TEMSW, 64,  2, 4, NBL_METHOD_TEMS,     0, 3, 2, 0, 3, 0, 1, "tems_wide",         true,  false, true,  false},
	{TEMSW, 64,  2, 4, NBL_METHOD_TEMS,     0, 5, 2, 0, 3, 0, 1, "tems",              false, false, true,  false},
	{TEMSW, 16,  2, 4, NBL_METHOD_TEMS,     0, 3, 2, 1, 3, 0, 1, "tems_wide_layered", false, false, true,  false},
	{TEMSW, 256, 2, 6, NBL_METHOD_TEMS,     0, 3, 2, 0, 0, 0, 1, "tems_wide",         false, false, true,  false},
	{TEMSW, 64,  2, 12, NBL_METHOD_TEMS,    0, 3, 2, 0, 1, 0, 1, "tems_wide",         false, false, true,  false},
	{TEMSW, 64,  2, 12, NBL_METHOD_TEMS,    0, 3, 2, 1, 0, 1, 1, "tems_wide_layered", false, false, true,  false},
	// nbl_create_bp_wide: the same
	{BPW,   64,  2, 6, NBL_METHOD_BP,       0, 0, 0, 0, 0, 0, 1, "bp_small",          true,  true,  true,  false},
	{BPW,   64,  2, 6, NBL_METHOD_BP,       0, 0, 0, 1, 0, 0, 1, "bp_layered",        false, false, true,  false},
	{BPW,   64,  2, 4, NBL_METHOD_BP,       0, 0, 0, 0, 3, 0, 1, "bp_wide",           true,  false, true,  false},
	{BPW,   64,  2, 4, NBL_METHOD_BP,       0, 0, 0, 1, 3, 0, 1, "bp_wide_layered",   false, false, true,  false},
	{BPW,   64,  2, 12, NBL_METHOD_BP,      0, 0, 0, 0, 0, 0, 1, "bp_wide",           false, false, true,  false},
	{BPW,   64,  2, 12, NBL_METHOD_BP,      0, 0, 0, 1, 2, 0, 1, "bp_wide_layered",   false, false, true,  false},
};

int main()
{
	int bad = 0, n = 0;
	for (const Row &r : rows) {
		const int M = 12, N = M * r.dc / r.dv;
		std::vector<int32_t> var_deg(N, r.dv), chk_deg(M, r.dc); // heap arrays of exactly N and M entries
		nbl_code_desc code{};
		code.N = N; code.M = M; code.q = r.q;
		code.var_deg = var_deg.data(); code.chk_deg = chk_deg.data();
		nbl_params prm{};
		prm.method = r.method;
		prm.ems_nm = r.nm; prm.ems_nc = r.nc; prm.tems_nr = r.nr; prm.tems_nc = r.nc;
		const NblShape s = nbl_shape(&code);
		NblPlanReq rq{};
		rq.kind = r.kind;
		rq.layered = r.layered != 0;
		rq.force_generic = r.force_generic;
		rq.record_state = r.record_state != 0;
		rq.small_on = r.small_on != 0;
		const NblPlan p = nbl_plan(s, prm, rq);
		const bool ok = s.maxdc == r.dc && s.min_dc == r.dc && s.maxdv == r.dv && s.mindv == r.dv && (1 << s.p) == r.q &&
		                !strcmp(nbl_plan_name(p), r.cn) && p.fusable == r.fusable && p.fused == r.fused && p.want_v2c == r.want_v2c && p.f32 == r.f32 &&
		                (!p.f32 || p.cn == (r.layered ? NBL_CN_FHT_LAYERED : NBL_CN_FHT)); // (a binary32 plan still says fht / fht_layered)
		if (!ok) {
			printf("row %d: got %s %d %d %d %d, want %s %d %d %d %d\n", n, nbl_plan_name(p), p.fusable, p.fused, p.want_v2c, p.f32, r.cn, r.fusable, r.fused,
			       r.want_v2c, r.f32);
			bad++;
		}
		n++;
	}
	for (int c = 0; c < NBL_CN_COUNT; c++) // every enumerator has a name
		if (!nbl_cn_name((NblCn)c) || !*nbl_cn_name((NblCn)c)) bad++;
	printf("%s %d\n", bad ? "FAILED" : "ok", n);
	return bad ? 1 : 0;
}
