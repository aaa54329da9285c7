// nbldpc_amd/host/nbldpc_host.cpp -- see nbldpc_host.h.
#include "nbldpc_host.h"
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

CNBLDPC::~CNBLDPC()
{
	if (dec) nbl_destroy(dec);
}

bool CNBLDPC::Initial(CSimulation &sim, int device, int fixed_iters)
{
	GFq = sim.GFq;
	maxIter = sim.maxIter;
	DecodeMethod = sim.decodeMethod;
	if (!GF.Initial(GFq)) { error = GF.error; return false; }

	// code file: "N M q" / "maxdv maxdc" / dv[N] / dc[M] / N rows of (check, h) / M rows of (var, h), 1-based (NBLDPC.cpp:147-205)
	std::ifstream f(sim.NonBinaryFileName);
	if (!f.is_open()) { error = "Cannot open " + sim.NonBinaryFileName; std::cerr << error << std::endl; return false; }
	f >> CodeLen >> ChkLen >> GFq >> maxVarDegree >> maxChkDegree;
	VarDegree.assign(CodeLen, 0);
	ChkDegree.assign(ChkLen, 0);
	for (auto &d : VarDegree) f >> d;
	for (auto &d : ChkDegree) f >> d;
	VarLink.assign(CodeLen, {}); VarLinkGFe.assign(CodeLen, {});
	ChkLink.assign(ChkLen, {}); ChkLinkGFe.assign(ChkLen, {});
	for (int n = 0; n < CodeLen; n++)
		for (int d = 0; d < VarDegree[n]; d++) { int c, h; f >> c >> h; VarLink[n].push_back(c - 1); VarLinkGFe[n].push_back(h); }
	for (int m = 0; m < ChkLen; m++)
		for (int d = 0; d < ChkDegree[m]; d++) { int v, h; f >> v >> h; ChkLink[m].push_back(v - 1); ChkLinkGFe[m].push_back(h); }
	if (!f) { error = "Malformed code file " + sim.NonBinaryFileName; std::cerr << error << std::endl; return false; }

	// every variable whose degree equals PuntureVarDegree is punctured (NBLDPC.cpp:163-176)
	PuncturePositionV.clear();
	for (int n = 0; n < CodeLen; n++)
		if (VarDegree[n] == sim.PuntureVarDegree) PuncturePositionV.push_back(n);
	PunctureLen = (int)PuncturePositionV.size();
	PuncturePosition = PuncturePositionV.data();

	if (sim.randomMsg && !InitialEncode()) return false;

	if (device < 0) return true; // host-only use (link-chain front-end, encoder): no decoder handle is created

	idd_passes = 1;
	idd_soft = NBL_SOFT_MAXLOG;
	if (const char *e = getenv("NBL_IDD_PASSES")) {
		char *end = nullptr;
		const long k = strtol(e, &end, 10);
		if (end == e || *end || k < 1 || k > 1000) {
			error = std::string("NBL_IDD_PASSES=") + e + ": the number of demapping passes must be an integer from 1 up";
			std::cerr << error << std::endl;
			return false;
		}
		idd_passes = (int)k;
	}
	if (const char *e = getenv("NBL_IDD_SOFT")) {
		const std::string v(e);
		if (v == "maxlog") idd_soft = NBL_SOFT_MAXLOG;
		else if (v == "logsum") idd_soft = NBL_SOFT_LOGSUM;
		else {
			error = "NBL_IDD_SOFT=" + v + ": unknown metric (maxlog, logsum)";
			std::cerr << error << std::endl;
			return false;
		}
	}

	// hand the graph and the parameters to the device library
	std::vector<int32_t> vchk, vh, cvar, ch;
	for (int n = 0; n < CodeLen; n++) for (int d = 0; d < VarDegree[n]; d++) { vchk.push_back(VarLink[n][d]); vh.push_back(VarLinkGFe[n][d]); }
	for (int m = 0; m < ChkLen; m++) for (int d = 0; d < ChkDegree[m]; d++) { cvar.push_back(ChkLink[m][d]); ch.push_back(ChkLinkGFe[m][d]); }
	nbl_code_desc code = {CodeLen, ChkLen, GFq, VarDegree.data(), ChkDegree.data(), vchk.data(), vh.data(), cvar.data(), ch.data()};
	std::vector<uint16_t> mul((size_t)GFq * GFq), inv(GFq, 0);
	for (int i = 0; i < GFq * GFq; i++) mul[i] = (uint16_t)GF.TableMultiply[i];
	for (int a = 1; a < GFq; a++) inv[a] = (uint16_t)GF.TableInverse[a];
	nbl_params p;
	memset(&p, 0, sizeof p);
	p.method = sim.decodeMethod;
	p.max_iter = sim.maxIter;
	p.ems_nm = sim.ems_nm; p.ems_nc = sim.ems_nc; p.ems_factor = sim.ems_factor; p.ems_offset = sim.ems_offset;
	p.tems_nr = sim.tems_nr; p.tems_nc = sim.tems_nc; p.tems_factor = sim.tems_factor; p.tems_offset = sim.tems_offset;
	p.fixed_iters = fixed_iters;
	p.poll_every = fixed_iters ? 0 : 2;
	p.max_batch = 0; // the workspace is sized at the first DecodingBatch call
	if (dec) { nbl_destroy(dec); dec = nullptr; }
	// basic-set T-EMS: its parameters go through the extension struct (NBLDPC.cpp:332-337)
	nbl_params_ext ext = {sim.bs_tems_nm, sim.bs_tems_nc, sim.bs_tems_factor, sim.bs_tems_offset};
	// OSD (method 6, or post-processing when OSD_order >= 0): the element matrices as CGF::Initial leaves them -- it reads q-2 of
	// the q-1 entries of ./SRC/Mat.Repr.GF.<q>.txt (GF.cpp:115-152), so alpha^(q-2)'s matrix stays zero.  (The reference's order-3
	// loop also prints "mm" for every frame, OSD.h:166; that debug print is not reproduced.)
	const bool osd = sim.decodeMethod == OSD_DECODE || sim.OSD_order >= 0;
	const bool minmax = sim.decodeMethod == MinMax_DECODE; // (through nbl_create_minmax, below)
	if (minmax && osd) {
		error = "DecodeMethod = 3: Min-Max decoding (nbl_create_minmax) has no OSD stage: set OSD_order below 0";
		std::cerr << error << std::endl;
		return false;
	}
	std::vector<uint8_t> gf_mat;
	if (osd && !LoadMatRepr(gf_mat)) return false;
	nbl_osd_params op = {sim.OSD_order, sim.OSD_flag, sim.OSD_factor, sim.crcLen, sim.crc_correctLen, gf_mat.data()};
	// NBL_SCHEDULE=layered: the layered (check-serial) schedule with the library's greedy layers in place of flooding (off by default;
	// EMS without OSD only -- nbl_create_layered says why).  NBL_SCHEDULE=layered-damped: the same through nbl_create_layered_ex with
	// NBL_LAYERED_DAMPED, which also serves T-EMS (its per-edge damping done by the check) and leaves EMS as it is; no OSD either.
	// NBL_SCHEDULE=layered-bp: log-QSPA (method 1) without OSD through nbl_create_layered_bp
	const char *sched = getenv("NBL_SCHEDULE");
	const bool damped = sched && std::string(sched) == "layered-damped";
	const bool lay_bp = sched && std::string(sched) == "layered-bp";
	const bool layered = damped || lay_bp || (sched && std::string(sched) == "layered");
	if (sched && !layered && std::string(sched) != "flooding") {
		error = std::string("NBL_SCHEDULE=") + sched + ": unknown schedule (flooding, layered, layered-damped, layered-bp)";
		std::cerr << error << std::endl;
		return false;
	}
	if (layered && osd) {
		error = lay_bp   ? "NBL_SCHEDULE=layered-bp: the layered log-QSPA schedule is defined for log-QSPA (method 1) without OSD only"
		        : damped ? "NBL_SCHEDULE=layered-damped: the damped layered schedule is defined for T-EMS (method 4) and EMS (method 2) without OSD only"
		                 : "NBL_SCHEDULE=layered: the layered schedule is defined for EMS (method 2) without OSD only";
		std::cerr << error << std::endl;
		return false;
	}
	// NBL_BP_CHECK=fht: the FHT sum-product check node in place of the exact one (nbl_create_fht; off by default, NBL_BP_CHECK=exact names
	// the default).  A log-QSPA profile (method 1) without OSD only; combines with NBL_SCHEDULE=flooding (or unset) and layered-bp
	const char *bpc = getenv("NBL_BP_CHECK");
	// NBL_BP_CHECK=fht32: the same in single precision (nbl_create_fht32: float messages, check degrees up to 8), under the same two schedules
	const bool fht = bpc && std::string(bpc) == "fht", fht32 = bpc && std::string(bpc) == "fht32";
	if (bpc && !fht && !fht32 && std::string(bpc) != "exact") {
		error = std::string("NBL_BP_CHECK=") + bpc + ": unknown check node (exact, fht, fht32)";
		std::cerr << error << std::endl;
		return false;
	}
	if ((fht || fht32) && (sim.decodeMethod != BP_DECODE || osd || (layered && !lay_bp))) {
		error = std::string("NBL_BP_CHECK=") + bpc + ": the FHT check node is defined for log-QSPA (method 1) without OSD only, under NBL_SCHEDULE=flooding or layered-bp";
		std::cerr << error << std::endl;
		return false;
	}
	// NBL_EMS_WIDE=1: EMS through nbl_create_ems_wide, which takes check degrees up to NBL_EMS_MAX_CHECK_DEGREE (off by default, NBL_EMS_WIDE=0
	// names the default).  An EMS profile (method 2) without OSD only; combines with NBL_SCHEDULE=flooding (or unset) and layered
	const char *wenv = getenv("NBL_EMS_WIDE");
	const bool wide = wenv && std::string(wenv) == "1";
	if (wenv && !wide && std::string(wenv) != "0") {
		error = std::string("NBL_EMS_WIDE=") + wenv + ": unknown value (0, 1)";
		std::cerr << error << std::endl;
		return false;
	}
	if (wide && (sim.decodeMethod != EMS_DECODE || osd || damped || lay_bp)) {
		error = "NBL_EMS_WIDE=1: the wide EMS decoder is defined for EMS (method 2) without OSD only, under NBL_SCHEDULE=flooding or layered";
		std::cerr << error << std::endl;
		return false;
	}
	// NBL_TEMS_WIDE=1: T-EMS through nbl_create_tems_wide, which takes check degrees up to NBL_TEMS_MAX_CHECK_DEGREE over any field (off by
	// default, NBL_TEMS_WIDE=0 names the default).  A T-EMS profile (method 4) without OSD only; combines with NBL_SCHEDULE=flooding (or
	// unset) and layered-damped
	const char *twenv = getenv("NBL_TEMS_WIDE");
	const bool twide = twenv && std::string(twenv) == "1";
	if (twenv && !twide && std::string(twenv) != "0") {
		error = std::string("NBL_TEMS_WIDE=") + twenv + ": unknown value (0, 1)";
		std::cerr << error << std::endl;
		return false;
	}
	if (twide && (sim.decodeMethod != T_EMS_DECODE || osd || wide || fht || fht32 || (layered && !damped))) {
		error = "NBL_TEMS_WIDE=1: the wide T-EMS decoder is defined for T-EMS (method 4) without OSD only, under NBL_SCHEDULE=flooding or layered-damped";
		std::cerr << error << std::endl;
		return false;
	}
	// NBL_BP_WIDE=1: exact log-QSPA through nbl_create_bp_wide, which takes check degrees up to NBL_BP_MAX_CHECK_DEGREE (off by default,
	// NBL_BP_WIDE=0 names the default).  A log-QSPA profile (method 1) without OSD only; combines with NBL_SCHEDULE=flooding (or unset) and
	// layered-bp; not with NBL_BP_CHECK=fht, which names another check node
	const char *bwenv = getenv("NBL_BP_WIDE");
	const bool bwide = bwenv && std::string(bwenv) == "1";
	if (bwenv && !bwide && std::string(bwenv) != "0") {
		error = std::string("NBL_BP_WIDE=") + bwenv + ": unknown value (0, 1)";
		std::cerr << error << std::endl;
		return false;
	}
	if (bwide && (fht || fht32)) {
		error = std::string("NBL_BP_WIDE=1 with NBL_BP_CHECK=") + bpc + ": the wide log-QSPA decoder runs the exact check node; the FHT check node takes checks up to degree 32 by itself";
		std::cerr << error << std::endl;
		return false;
	}
	if (bwide && (sim.decodeMethod != BP_DECODE || osd || wide || twide || (layered && !lay_bp))) {
		error = "NBL_BP_WIDE=1: the wide log-QSPA decoder is defined for log-QSPA (method 1) without OSD only, under NBL_SCHEDULE=flooding or layered-bp";
		std::cerr << error << std::endl;
		return false;
	}
	// NBL_FHT32_WIDE=1 (with NBL_BP_CHECK=fht32 only): single-precision FHT through nbl_create_fht32_wide, which takes check degrees up to
	// NBL_FHT32_MAX_CHECK_DEGREE (off by default, NBL_FHT32_WIDE=0 names the default); the same two schedules
	const char *fwenv = getenv("NBL_FHT32_WIDE");
	const bool fwide = fwenv && std::string(fwenv) == "1";
	if (fwenv && !fwide && std::string(fwenv) != "0") {
		error = std::string("NBL_FHT32_WIDE=") + fwenv + ": unknown value (0, 1)";
		std::cerr << error << std::endl;
		return false;
	}
	if (fwide && !fht32) {
		error = "NBL_FHT32_WIDE=1: the wide single-precision FHT decoder goes with NBL_BP_CHECK=fht32 (log-QSPA, method 1, without OSD, under NBL_SCHEDULE=flooding or layered-bp)";
		std::cerr << error << std::endl;
		return false;
	}
	// DecodeMethod = 3: Min-Max through nbl_create_minmax, shaping from the profile's EMS factor / offset, under NBL_SCHEDULE=flooding (or
	// unset) and layered.  No switch: nothing else can be meant by method 3.  No OSD, and none of the switches of the other kinds
	if (minmax && (damped || lay_bp || fht || fht32 || wide || twide || bwide || fwide)) {
		error = "DecodeMethod = 3: the Min-Max decoder is defined for Min-Max (method 3) without OSD only, under NBL_SCHEDULE=flooding or layered";
		std::cerr << error << std::endl;
		return false;
	}
	nbl_status st = minmax    ? nbl_create_minmax(&code, mul.data(), inv.data(), &p, nullptr, layered ? NBL_MINMAX_LAYERED : 0u, device, &dec)
	                : bwide   ? nbl_create_bp_wide(&code, mul.data(), inv.data(), &p, nullptr, lay_bp ? NBL_BP_WIDE_LAYERED : 0u, device, &dec)
	                : fwide   ? nbl_create_fht32_wide(&code, mul.data(), inv.data(), &p, nullptr, lay_bp ? NBL_FHT32_WIDE_LAYERED : 0u, device, &dec)
	                : twide   ? nbl_create_tems_wide(&code, mul.data(), inv.data(), &p, nullptr, damped ? NBL_TEMS_WIDE_LAYERED : 0u, device, &dec)
	                : wide    ? nbl_create_ems_wide(&code, mul.data(), inv.data(), &p, nullptr, layered ? NBL_EMS_WIDE_LAYERED : 0u, device, &dec)
	                : fht32   ? nbl_create_fht32(&code, mul.data(), inv.data(), &p, nullptr, lay_bp ? NBL_FHT32_LAYERED : 0u, device, &dec)
	                : fht     ? nbl_create_fht(&code, mul.data(), inv.data(), &p, nullptr, lay_bp ? NBL_FHT_LAYERED : 0u, device, &dec)
	                : lay_bp  ? nbl_create_layered_bp(&code, mul.data(), inv.data(), &p, nullptr, device, &dec)
	                : damped  ? nbl_create_layered_ex(&code, mul.data(), inv.data(), &p, nullptr, NBL_LAYERED_DAMPED, device, &dec)
	                : layered ? nbl_create_layered(&code, mul.data(), inv.data(), &p, nullptr, device, &dec)
	                          : nbl_create_osd(&code, mul.data(), inv.data(), &p, sim.decodeMethod == BS_TEMS_DECODE ? &ext : nullptr,
	                                           osd ? &op : nullptr, device, &dec);
	if (st != NBL_OK) {
		error = nbl_last_error(nullptr);
		std::cerr << error << std::endl; // the reference prints and exits for its own configuration errors (NBLDPC.cpp:284-285)
		return false;
	}
	return true;
}

// [q][p][p] GFElement[e].ValueMatric as CGF::Initial reads them (GF.cpp:115-152): q-2 entries "A^k --> order: k poly: e" each
// followed by p rows of p bits; element 0 and the element never read keep zero matrices
bool CNBLDPC::LoadMatRepr(std::vector<uint8_t> &m)
{
	int p = 0;
	while ((1 << p) < GFq) p++;
	const std::string name = "./SRC/Mat.Repr.GF." + std::to_string(GFq) + ".txt";
	std::ifstream f(name);
	if (!f.is_open()) { error = "Cannot open " + name; std::cerr << error << std::endl; return false; }
	std::string rub;
	std::getline(f, rub);
	m.assign((size_t)GFq * p * p, 0);
	for (int k = 0; k < GFq - 2; k++) {
		int order = 0, e = 0;
		f >> rub >> rub >> rub >> order >> rub >> e;
		if (!f || e <= 0 || e >= GFq) { error = "Malformed " + name; std::cerr << error << std::endl; return false; }
		for (int i = 0; i < p * p; i++) {
			int bit = 0;
			f >> bit;
			m[(size_t)e * p * p + i] = (uint8_t)bit;
		}
	}
	if (!f) { error = "Malformed " + name; std::cerr << error << std::endl; return false; }
	return true;
}

// Systematic form by Gauss elimination from the last row up, pivot in column (row + N - M); a missing pivot is fetched from
// a row above, else from a column to the left (the column swap is recorded and undone after encoding).  NBLDPC.cpp:1474-1538.
bool CNBLDPC::InitialEncode()
{
	const int N = CodeLen, M = ChkLen;
	std::vector<std::vector<int>> H(M, std::vector<int>(N, 0));
	for (int m = 0; m < M; m++)
		for (size_t d = 0; d < ChkLink[m].size(); d++) H[m][ChkLink[m][d]] = ChkLinkGFe[m][d];
	swap_src.clear(); swap_dst.clear();
	for (int row = M - 1; row >= 0; row--) {
		const int col = row + N - M;
		if (H[row][col] == 0) {
			bool found = false;
			for (int up = row - 1; up >= 0 && !found; up--)
				if (H[up][col] != 0) { std::swap(H[row], H[up]); found = true; }
			for (int left = col - 1; left >= 0 && !found; left--)
				if (H[row][left] != 0) {
					for (int m = 0; m < M; m++) std::swap(H[m][col], H[m][left]);
					swap_src.push_back(col); swap_dst.push_back(left);
					found = true;
				}
			if (!found) { error = "NB matrix is not full rank"; std::cerr << error << std::endl; return false; }
		}
		const int hinv = GF.GFInverse(H[row][col]);
		for (int up = row - 1; up >= 0; up--)
			if (H[up][col] != 0) {
				const int x = GF.GFMultiply(hinv, H[up][col]);
				for (int c = 0; c < N; c++) H[up][c] = GF.GFAdd(H[up][c], GF.GFMultiply(x, H[row][c]));
			}
		for (int c = 0; c <= col; c++) H[row][c] = GF.GFMultiply(H[row][c], hinv);
	}
	enc_link.assign(M, {}); enc_coef.assign(M, {});
	for (int p = 0; p < M; p++)
		for (int c = 0; c < N - M + p; c++)
			if (H[p][c] != 0) { enc_link[p].push_back(c); enc_coef[p].push_back(H[p][c]); }
	return true;
}

int CNBLDPC::Encode(int *msg_sym, int *code_sym) // NBLDPC.cpp:562-604
{
	const int K = CodeLen - ChkLen;
	for (int c = 0; c < K; c++) code_sym[c] = msg_sym[c];
	for (int c = K; c < CodeLen; c++) code_sym[c] = 0;
	for (int p = 0; p < ChkLen; p++) {
		int acc = 0;
		for (size_t d = 0; d < enc_link[p].size(); d++) acc = GF.GFAdd(acc, GF.GFMultiply(enc_coef[p][d], code_sym[enc_link[p][d]]));
		code_sym[K + p] = acc;
	}
	for (int k = (int)swap_src.size() - 1; k >= 0; k--) std::swap(code_sym[swap_src[k]], code_sym[swap_dst[k]]);
	for (int c = 0; c < K; c++) msg_sym[c] = code_sym[c];
	return 0;
}

bool CNBLDPC::Generator(std::vector<uint16_t> &gen)
{
	const int N = CodeLen, K = CodeLen - ChkLen;
	if (enc_link.empty() && !InitialEncode()) return false;
	gen.assign((size_t)N * K, 0);
	std::vector<int> msg(K), cw(N);
	for (int k = 0; k < K; k++) {
		std::fill(msg.begin(), msg.end(), 0);
		msg[k] = 1;
		Encode(msg.data(), cw.data());
		for (int n = 0; n < N; n++) gen[(size_t)n * K + k] = (uint16_t)cw[n];
	}
	return true;
}

int CNBLDPC::SetTransmitter(const uint16_t *gen, int crc_len, int random_msg, int parallel, int mod_order, int n_mod_sym)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	nbl_tx_desc tx = {gen, crc_len, random_msg, parallel, PuncturePositionV.data(), PunctureLen, mod_order, n_mod_sym};
	nbl_status st = nbl_set_transmitter(dec, &tx);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::TransmitBatch(int slot, const uint16_t *pn_state, const unsigned int *lane_state, double sigma, int B)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	nbl_status st = nbl_transmit_batch(dec, slot, pn_state, lane_state, sigma, B);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::CountErrors(int slot, int B, int *err_sym, int *err_bit, uint8_t *crc_ok)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	nbl_status st = nbl_count_errors(dec, slot, B, err_sym, err_bit, crc_ok);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::DecodingBatch(const double *L_ch, int B, int *out, uint8_t *converged, int *iters)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	nbl_status st = nbl_decode_batch(dec, L_ch, B, out, converged, iters);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::SetDemodulator(int mod_order, int n_mod_sym, const double *constellation, const int *src, int metric)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	if (idd_passes > 1 && (mod_order == 2 || mod_order == GFq)) {
		error = "NBL_IDD_PASSES=" + std::to_string(idd_passes) + ": iterative demapping needs the general demodulator (a modulation order other than 2 and GFq); "
		        "this one has no foreign bits and every pass would be the same decode";
		std::cerr << error << std::endl;
		return -1;
	}
	nbl_demod_desc dm = {mod_order, n_mod_sym, constellation, src};
	nbl_demod_ext ext = {metric, 0}; // orders 2 and GFq: the two reference-pinned paths, the metric is not read
	nbl_status st = nbl_set_demodulator_ex(dec, &dm, &ext);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::SetFading(int model, int coherence)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	const nbl_fading_desc f = {model, coherence};
	nbl_status st = nbl_set_fading(dec, &f);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::DecodingBatchSamples(const double *rx, double sigma, int B, int *out, uint8_t *converged, int *iters, const double *gain)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	const nbl_idd_params idd = {idd_passes, idd_soft};
	nbl_status st;
	if (gain)
		st = idd_passes > 1 ? nbl_decode_batch_samples_idd_csi(dec, rx, gain, sigma, B, &idd, out, converged, iters, nullptr)
		                    : nbl_decode_batch_samples_csi(dec, rx, gain, nullptr, sigma, B, out, converged, iters);
	else
		st = idd_passes > 1 ? nbl_decode_batch_samples_idd(dec, rx, sigma, B, &idd, out, converged, iters, nullptr)
		                    : nbl_decode_batch_samples(dec, rx, sigma, B, out, converged, iters);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::DecodingBatchBits(const double *bit_llr, int B, int *out, uint8_t *converged, int *iters)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	nbl_status st = nbl_decode_batch_bits(dec, bit_llr, B, out, converged, iters);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::SoftOutput(int metric, double *sym_llr, double *bit_llr)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	nbl_status st = nbl_soft_output(dec, metric, sym_llr, bit_llr);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::DecodingBatchNoise(const unsigned char *tx_index, const unsigned int *lane_state, double sigma, int B, int *out, uint8_t *converged, int *iters)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	nbl_status st = nbl_decode_batch_noise(dec, tx_index, lane_state, sigma, B, out, converged, iters);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::ChannelBatch(int slot, const unsigned char *tx_index, const unsigned int *lane_state, double sigma, int B)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	nbl_status st = nbl_channel_batch(dec, slot, tx_index, lane_state, sigma, B);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::DecodingBatchResident(int slot, double sigma, int B, int *out, uint8_t *converged, int *iters)
{
	if (!dec) { error = "decoder not initialised"; return -1; }
	const nbl_idd_params idd = {idd_passes, idd_soft};
	nbl_status st = idd_passes > 1 ? nbl_decode_batch_resident_idd(dec, slot, sigma, B, &idd, out, converged, iters, nullptr)
	                               : nbl_decode_batch_resident(dec, slot, sigma, B, out, converged, iters);
	if (st != NBL_OK) { error = nbl_last_error(dec); std::cerr << error << std::endl; return (int)st; }
	return 0;
}

int CNBLDPC::Decoding(double **L_ch, int *DecodeOutput, int *, int *) // NBLDPC.cpp:607
{
	std::vector<double> flat((size_t)CodeLen * (GFq - 1));
	for (int n = 0; n < CodeLen; n++) memcpy(&flat[(size_t)n * (GFq - 1)], L_ch[n], sizeof(double) * (GFq - 1));
	uint8_t ok = 0;
	if (DecodingBatch(flat.data(), 1, DecodeOutput, &ok, nullptr) != 0) return 0;
	return ok;
}
