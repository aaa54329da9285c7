// tests/bstems_check.cpp -- CPU restatement of the reference's basic-set T-EMS decode (decode method 7), for tests only.
//
// Written from the description in DESIGN.md section 3 ("BS-TEMS"), not from the reference's text.  Per iteration:
//   a-posteriori sum (L_ch, then the variable's edges in order), hard decision, syndrome (return at the first zero syndrome),
//   v2c = post - c2v with 0.25 / 0.75 damping when the v2c decision changes, then per check:
//   1. beta / syndrome / delta-domain dU and, per symbol, the two smallest columns (stable: ties go to the lower column);
//   2. the basic set: LLV[s] = dU[Min[s][0]][s]; symbols ordered by LLV; nm > p: the nm first non-zero entries of that
//      order; nm <= p: a greedy GF(2) basis along it (each symbol not in the span of those already taken);
//   3. a DFS over the nm elements (include before exclude, an element whose column is taken is skipped, at most nc columns);
//      a leaf sets dW[xor] / Eta[xor] when its cost is strictly below the current dW[xor]; dW[0] = 0, Eta[0] = 0 beforehand;
//   4. the T-EMS output stage with the BS-TEMS factor / offset.
// Two modes:
//   LITERAL   (0): the order of step 2 is std::sort with the reference's comparator (LLV only), the DFS keeps a running sum
//                  (+= on the way in, -= on the way out) -- what the compiled reference computes, bit for bit;
//   CANONICAL (1): the order is (LLV, symbol), a leaf's cost is the left-to-right sum of its elements in element order --
//                  what the GPU kernel (nbldpc_amd/csrc/nbl_cn_bstems.hip) computes, bit for bit.
// fixed_iters = 1 keeps iterating after the first zero syndrome (outputs frozen there), like the library's throughput mode.
//
// usage: bstems_check <in.bin> <out.bin> [threads]      (layout: tests/bstems_util.py)
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

struct Graph {
	int N, M, q, E, p, maxdc;
	std::vector<int> voff, coff, v_chk, v_ce, c_var, c_h, c_ve; // v_ce: var-major edge -> check-major slot; c_ve: inverse
	std::vector<int> mul, inv;
	int MUL(int a, int b) const { return mul[(size_t)a * q + b]; }
};

struct Prm {
	int nm, nc, max_iter, mode, fixed_iters;
	double factor, offset;
};

struct Dec {
	const Graph *g;
	Prm prm;
	int w;
	std::vector<double> post, v2c, c2v, old, dU, dW, lc, llv, el_L;
	std::vector<int> dec, beta, tmin0, tmin1, eta, cand, el_q, el_col;
	std::vector<unsigned char> upd, colsel;
	// running state of the LITERAL DFS
	double run_sum;
	int run_sym, run_diff;

	explicit Dec(const Graph *g_, const Prm &p) : g(g_), prm(p), w(g_->q - 1)
	{
		const int q = g->q, md = g->maxdc;
		post.assign((size_t)g->N * w, 0.0);
		v2c.assign((size_t)g->E * w, 0.0);
		c2v.assign((size_t)g->E * w, 0.0);
		old.assign(w, 0.0);
		dU.assign((size_t)md * q, 0.0);
		dW.assign(q, 0.0);
		lc.assign(q, 0.0);
		llv.assign(q, 0.0);
		el_L.assign(q, 0.0);
		dec.assign(g->N, 0);
		beta.assign(md, 0);
		tmin0.assign(q, 0);
		tmin1.assign(q, 0);
		eta.assign((size_t)q * md, 0);
		cand.assign(md, 0);
		el_q.assign(q, 0);
		el_col.assign(q, 0);
		upd.assign(q, 0);
		colsel.assign(md, 0);
	}

	static int decide(const double *L, int w)
	{
		double best = 0;
		int arg = 0;
		for (int a = 0; a < w; a++)
			if (L[a] > best) { best = L[a]; arg = a + 1; }
		return arg;
	}

	double shape(double y) const
	{
		y = y / prm.factor;
		if (y < -1 * prm.offset) return y + prm.offset;
		if (y > prm.offset) return y - prm.offset;
		return 0;
	}

	void leaf(int sym, double cost)
	{
		if (cost < dW[sym]) {
			dW[sym] = cost;
			for (int d = 0; d < g->maxdc; d++) eta[(size_t)sym * g->maxdc + d] = cand[d];
		}
	}

	// LITERAL: running sum, as the reference keeps it
	void dfs_literal(int k, int end)
	{
		if (k > end) { leaf(run_sym, run_sum); return; }
		const int col = el_col[k];
		if (colsel[col]) { dfs_literal(k + 1, end); return; }
		run_diff += 1;
		if (run_diff <= prm.nc) {
			colsel[col] = 1;
			run_sym ^= el_q[k];
			run_sum += el_L[k];
			cand[col] = el_q[k];
			dfs_literal(k + 1, end);
			run_sym ^= el_q[k];
			run_sum -= el_L[k];
			colsel[col] = 0;
			run_diff -= 1;
			cand[col] = 0;
			dfs_literal(k + 1, end);
		} else {
			run_diff -= 1;
			cand[col] = 0;
			dfs_literal(k + 1, end);
		}
	}

	// CANONICAL: a leaf's cost is the left-to-right sum of its elements
	void dfs_canonical(int k, int end, int sym, double vsum, int diff)
	{
		if (k > end) { leaf(sym, vsum); return; }
		const int col = el_col[k];
		if (colsel[col]) { dfs_canonical(k + 1, end, sym, vsum, diff); return; }
		if (diff + 1 <= prm.nc) {
			colsel[col] = 1;
			cand[col] = el_q[k];
			dfs_canonical(k + 1, end, sym ^ el_q[k], vsum + el_L[k], diff + 1);
			colsel[col] = 0;
			cand[col] = 0;
		}
		dfs_canonical(k + 1, end, sym, vsum, diff);
	}

	void check(int m)
	{
		const Graph &G = *g;
		const int q = G.q, md = G.maxdc, c0 = G.coff[m], dc = G.coff[m + 1] - c0;
		int syn = 0;
		// 1. beta, syndrome, dU
		for (int k = 0; k < dc; k++) {
			const double *V = &v2c[(size_t)G.c_ve[c0 + k] * w];
			const int h = G.c_h[c0 + k];
			double best = 0;
			int arg = 0;
			for (int a = 1; a < q; a++)
				if (V[a - 1] > best) { best = V[a - 1]; arg = G.MUL(a, h); }
			beta[k] = arg;
			syn ^= arg;
		}
		for (int k = 0; k < dc; k++) {
			const double *V = &v2c[(size_t)G.c_ve[c0 + k] * w];
			const int hi = G.inv[G.c_h[c0 + k]], bp = G.MUL(hi, beta[k]);
			const double mx = bp ? V[bp - 1] : 0;
			dU[(size_t)k * q + beta[k]] = mx - 0;
			for (int x = 1; x < q; x++) dU[(size_t)k * q + (x ^ beta[k])] = mx - V[G.MUL(hi, x) - 1];
		}
		// per symbol: the two smallest columns of a stable ascending order
		for (int s = 0; s < q; s++) {
			int b0 = 0, b1 = -1;
			for (int k = 1; k < dc; k++) {
				const double u = dU[(size_t)k * q + s];
				if (u < dU[(size_t)b0 * q + s]) { b1 = b0; b0 = k; }
				else if (b1 < 0 || u < dU[(size_t)b1 * q + s]) b1 = k;
			}
			tmin0[s] = b0;
			tmin1[s] = b1;
			llv[s] = dU[(size_t)b0 * q + s];
		}
		// the all-zero configuration: dW[0] = 0, Eta[0] = 0, every other dW unreached
		for (int s = 0; s < q; s++) dW[s] = DBL_MAX;
		dW[0] = 0.0;
		for (int d = 0; d < dc; d++) { eta[d] = 0; cand[d] = 0; }
		// 2. the basic set
		std::vector<int> order(q);
		for (int s = 0; s < q; s++) order[s] = s;
		const std::vector<double> &L = llv;
		if (prm.mode == 0) std::sort(order.begin(), order.end(), [&L](int a, int b) { return L[a] < L[b]; });
		else std::sort(order.begin(), order.end(), [&L](int a, int b) { return L[a] < L[b] || (L[a] == L[b] && a < b); });
		int nel = 0;
		if (prm.nm > G.p) {
			for (int i = 0; i < q - 1; i++) { el_q[i] = order[i + 1]; el_col[i] = tmin0[order[i + 1]]; el_L[i] = llv[order[i + 1]]; }
			nel = q - 1;
		} else {
			std::vector<unsigned char> avail(q, 1);
			std::vector<int> span;
			avail[0] = 0;
			auto take = [&](int s) {
				el_q[nel] = s; el_col[nel] = tmin0[s]; el_L[nel] = llv[s]; nel++;
				const size_t n = span.size();
				for (size_t j = 0; j < n; j++) { span.push_back(s ^ span[j]); avail[s ^ span[j]] = 0; }
				span.push_back(s);
				avail[s] = 0;
			};
			take(order[1]);
			for (int i = 2; i < q && (int)span.size() < q - 1; i++)
				if (avail[order[i]]) take(order[i]);
		}
		(void)nel;
		// 3. configurations over the first nm elements
		for (int d = 0; d < md; d++) colsel[d] = 0;
		if (prm.mode == 0) {
			run_sum = 0.0; run_sym = 0; run_diff = 0;
			dfs_literal(0, prm.nm - 1);
		} else {
			dfs_canonical(0, prm.nm - 1, 0, 0.0, 0);
		}
		// 4. extrinsic output per edge
		for (int k = 0; k < dc; k++) {
			const int hi = G.inv[G.c_h[c0 + k]], bsyn = syn ^ beta[k];
			for (int s = 0; s < q; s++) { lc[s] = DBL_MAX; upd[s] = 0; }
			for (int e = 0; e < q; e++) {
				const int dev = eta[(size_t)e * md + k], tgt = e ^ dev;
				const double c = dW[e] - dU[(size_t)k * q + dev];
				if (lc[tgt] > c) { lc[tgt] = c; upd[tgt] = 1; }
			}
			for (int s = 0; s < q; s++)
				if (!upd[s]) lc[s] = (k == tmin0[s]) ? dU[(size_t)tmin1[s] * q + s] : dU[(size_t)tmin0[s] * q + s];
			const double L0 = -1.0 * lc[bsyn];
			double *C = &c2v[(size_t)(c0 + k) * w];
			for (int e = 0; e < q; e++) {
				if (e == bsyn) continue;
				C[G.MUL(hi, e ^ bsyn) - 1] = shape(-1.0 * lc[e] - L0);
			}
		}
	}

	int decode(const double *L_ch, int *out, int *iters)
	{
		const Graph &G = *g;
		int frozen = 0, it = 0;
		for (int n = 0; n < G.N; n++)
			for (int e = G.voff[n]; e < G.voff[n + 1]; e++) memcpy(&v2c[(size_t)e * w], L_ch + (size_t)n * w, sizeof(double) * w);
		std::fill(c2v.begin(), c2v.end(), 0.0);
		*iters = prm.max_iter;
		while (it++ < prm.max_iter) {
			for (int n = 0; n < G.N; n++) {
				double *P = &post[(size_t)n * w];
				memcpy(P, L_ch + (size_t)n * w, sizeof(double) * w);
				for (int e = G.voff[n]; e < G.voff[n + 1]; e++) {
					const double *C = &c2v[(size_t)G.v_ce[e] * w];
					for (int a = 0; a < w; a++) P[a] = P[a] + C[a];
				}
				dec[n] = decide(P, w);
			}
			if (!frozen) memcpy(out, dec.data(), sizeof(int) * G.N);
			int ok = 1;
			for (int m = 0; m < G.M && ok; m++) {
				int s = 0;
				for (int ce = G.coff[m]; ce < G.coff[m + 1]; ce++) s ^= G.MUL(G.c_h[ce], dec[G.c_var[ce]]);
				if (s) ok = 0;
			}
			if (ok && !frozen) {
				frozen = 1;
				*iters = it;
				if (!prm.fixed_iters) return 1;
			}
			for (int n = 0; n < G.N; n++) {
				const double *P = &post[(size_t)n * w];
				for (int e = G.voff[n]; e < G.voff[n + 1]; e++) {
					double *V = &v2c[(size_t)e * w];
					const double *C = &c2v[(size_t)G.v_ce[e] * w];
					const int before = decide(V, w);
					memcpy(old.data(), V, sizeof(double) * w);
					for (int a = 0; a < w; a++) V[a] = P[a] - C[a];
					if (decide(V, w) != before)
						for (int a = 0; a < w; a++) V[a] = 0.25 * old[a] + 0.75 * V[a];
				}
			}
			for (int m = 0; m < G.M; m++) check(m);
		}
		return frozen;
	}
};

template <typename T> static void rd(FILE *f, T *p, size_t n)
{
	if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
}

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: bstems_check in.bin out.bin [threads]\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	int32_t h[12];
	rd(f, h, 12);
	Graph G;
	G.N = h[0]; G.M = h[1]; G.q = h[2]; G.E = h[3];
	Prm P;
	P.nm = h[4]; P.nc = h[5]; P.max_iter = h[6]; P.mode = h[7]; P.fixed_iters = h[8];
	const int B = h[9], nstate = h[10];
	rd(f, &P.factor, 1);
	rd(f, &P.offset, 1);
	std::vector<int> vdeg(G.N), cdeg(G.M), vchk(G.E), vh(G.E), cvar(G.E), ch(G.E);
	rd(f, vdeg.data(), G.N); rd(f, cdeg.data(), G.M);
	rd(f, vchk.data(), G.E); rd(f, vh.data(), G.E); rd(f, cvar.data(), G.E); rd(f, ch.data(), G.E);
	G.mul.resize((size_t)G.q * G.q); G.inv.resize(G.q);
	rd(f, G.mul.data(), G.mul.size()); rd(f, G.inv.data(), G.q);
	std::vector<int> sidx(nstate);
	rd(f, sidx.data(), nstate);
	const int w = G.q - 1;
	std::vector<double> Lch((size_t)B * G.N * w);
	rd(f, Lch.data(), Lch.size());
	fclose(f);
	G.p = 0;
	while ((1 << G.p) < G.q) G.p++;
	G.voff.assign(G.N + 1, 0); G.coff.assign(G.M + 1, 0);
	for (int n = 0; n < G.N; n++) G.voff[n + 1] = G.voff[n] + vdeg[n];
	G.maxdc = 0;
	for (int m = 0; m < G.M; m++) { G.coff[m + 1] = G.coff[m] + cdeg[m]; G.maxdc = std::max(G.maxdc, cdeg[m]); }
	G.c_var = cvar; G.c_h = ch; G.v_chk = vchk;
	G.v_ce.assign(G.E, -1); G.c_ve.assign(G.E, -1);
	for (int n = 0; n < G.N; n++)
		for (int e = G.voff[n]; e < G.voff[n + 1]; e++) {
			const int m = vchk[e];
			for (int ce = G.coff[m]; ce < G.coff[m + 1]; ce++)
				if (cvar[ce] == n) G.v_ce[e] = ce; // last match wins (the reference's cross index)
		}
	for (int m = 0; m < G.M; m++)
		for (int ce = G.coff[m]; ce < G.coff[m + 1]; ce++) {
			const int n = cvar[ce];
			for (int e = G.voff[n]; e < G.voff[n + 1]; e++)
				if (vchk[e] == m) G.c_ve[ce] = e;
		}

	std::vector<int> out((size_t)B * G.N), ret(B), its(B);
	std::vector<char> want(B, 0);
	for (int b : sidx) want[b] = 1;
	std::vector<double> st((size_t)nstate * ((size_t)G.N * w + 2 * (size_t)G.E * w));
	std::vector<int> spos(B, -1);
	for (int i = 0; i < nstate; i++) spos[sidx[i]] = i;
	int nt = argc > 3 ? atoi(argv[3]) : 1;
	if (nt < 1) nt = 1;
	std::vector<std::thread> th;
	for (int t = 0; t < nt; t++)
		th.emplace_back([&, t]() {
			Dec d(&G, P);
			for (int b = t; b < B; b += nt) {
				ret[b] = d.decode(&Lch[(size_t)b * G.N * w], &out[(size_t)b * G.N], &its[b]);
				if (spos[b] < 0) continue;
				double *o = &st[(size_t)spos[b] * ((size_t)G.N * w + 2 * (size_t)G.E * w)];
				memcpy(o, d.post.data(), sizeof(double) * G.N * w);
				memcpy(o + (size_t)G.N * w, d.v2c.data(), sizeof(double) * G.E * w);
				double *c = o + (size_t)G.N * w + (size_t)G.E * w;
				for (int e = 0; e < G.E; e++) memcpy(c + (size_t)e * w, &d.c2v[(size_t)G.v_ce[e] * w], sizeof(double) * w);
			}
		});
	for (auto &t : th) t.join();
	FILE *o = fopen(argv[2], "wb");
	if (!o) return 2;
	fwrite(out.data(), 4, out.size(), o);
	fwrite(ret.data(), 4, ret.size(), o);
	fwrite(its.data(), 4, its.size(), o);
	fwrite(st.data(), 8, st.size(), o);
	fclose(o);
	return 0;
}
