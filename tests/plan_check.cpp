// tests/plan_check.cpp -- nbl_shape() and nbl_plan() (nbldpc_amd/csrc/nbl_plan.cpp) in a stand-alone host program, for a build with
// -fsanitize=address,undefined: a handful of rows of tests/golden/cn_plan_table.json on (dv, dc)-regular shapes, with degree arrays
// that end exactly where the code description says (a read past N or M entries is an error the sanitizer reports).
// The nbl_*_applicable predicates come from the product library.  Prints "ok <rows>"; exit status 1 on a wrong row.
#include <cstdio>
#include <cstring>
#include <vector>
#include "nbl_plan.h"

struct Row {
	int q, dv, dc, method, nm, nc, nr, layered, force_generic, record_state, small_on;
	const char *cn;
	bool fusable, fused, want_v2c;
};

static const Row rows[] = {
	// q  dv dc  method             nm  nc nr lay fg rs small  kernel          fusable fused  v2c
	{256, 2, 4, NBL_METHOD_EMS,     32, 3, 0, 0, 0, 0, 1, "ems256",       true,  true,  false},
	{256, 2, 4, NBL_METHOD_EMS,     32, 3, 0, 0, 1, 0, 1, "ems",          true,  false, true},
	{256, 2, 4, NBL_METHOD_EMS,     32, 3, 0, 0, 2, 0, 1, "ems256",       true,  false, true},
	{256, 2, 4, NBL_METHOD_EMS,     32, 3, 0, 0, 0, 1, 1, "ems256",       true,  true,  true},
	{256, 2, 4, NBL_METHOD_EMS,     65, 3, 0, 0, 0, 0, 1, "ems",          false, false, true},
	{256, 3, 4, NBL_METHOD_TEMS,     0, 3, 2, 0, 0, 0, 1, "tems256",      false, false, true},
	{64,  3, 4, NBL_METHOD_BP,       0, 0, 0, 0, 0, 0, 1, "bp64",         false, false, true},
	{64,  2, 6, NBL_METHOD_BP,       0, 0, 0, 0, 0, 0, 1, "bp_small",     true,  true,  true},
	{64,  2, 6, NBL_METHOD_BP,       0, 0, 0, 0, 0, 0, 0, "bp",           false, false, true},
	{64,  2, 6, NBL_METHOD_EMS,      8, 2, 0, 0, 0, 0, 1, "ems64",        true,  true,  false},
	{64,  2, 6, NBL_METHOD_EMS,      8, 2, 0, 0, 0, 0, 0, "ems",          false, false, true},
	{64,  2, 4, NBL_METHOD_TEMS,     0, 3, 2, 0, 0, 0, 0, "tems64",       true,  true,  true},
	{16,  2, 4, NBL_METHOD_EMS,      8, 2, 0, 0, 0, 0, 1, "ems_small",    true,  true,  false},
	{16,  4, 4, NBL_METHOD_TEMS,     0, 3, 2, 0, 0, 0, 1, "tems_small",   false, false, true},
	{16,  2, 4, NBL_METHOD_EMS,      8, 2, 0, 1, 0, 0, 1, "ems_layered",  false, false, false},
	{16,  2, 4, NBL_METHOD_TEMS,     0, 3, 2, 1, 0, 0, 1, "tems_layered", false, false, true},
	{16,  2, 4, NBL_METHOD_BS_TEMS,  4, 2, 0, 0, 0, 0, 1, "bstems",       false, false, true},
	{16,  2, 4, NBL_METHOD_OSD,      0, 0, 0, 0, 0, 0, 1, "none",         false, false, true},
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
		nbl_params_ext ext{};
		ext.bs_nm = r.nm; ext.bs_nc = r.nc;
		const NblShape s = nbl_shape(&code);
		const NblPlan p = nbl_plan(s, prm, ext, r.layered != 0, r.force_generic, r.record_state != 0, r.small_on != 0);
		const bool ok = s.maxdc == r.dc && s.min_dc == r.dc && s.maxdv == r.dv && s.mindv == r.dv && (1 << s.p) == r.q &&
		                !strcmp(nbl_cn_name(p.cn), r.cn) && p.fusable == r.fusable && p.fused == r.fused && p.want_v2c == r.want_v2c;
		if (!ok) {
			printf("row %d: got %s %d %d %d, want %s %d %d %d\n", n, nbl_cn_name(p.cn), p.fusable, p.fused, p.want_v2c, r.cn, r.fusable, r.fused, r.want_v2c);
			bad++;
		}
		n++;
	}
	for (int c = 0; c < NBL_CN_COUNT; c++) // every enumerator has a name
		if (!nbl_cn_name((NblCn)c) || !*nbl_cn_name((NblCn)c)) bad++;
	printf("%s %d\n", bad ? "FAILED" : "ok", n);
	return bad ? 1 : 0;
}
