// tests/osd_check.cpp -- CPU restatement of the reference's ordered-statistics decoding (OSD.h: Decoding_OSD_bit, OSD_permute,
// H_GaussEliminate_bit, OSD_Encode_bit, compute_min_distance_bit, CRCMatrixGen, G_GaussEliminate_bit) for the OSD tests.
//
// Written from the reference's semantics, independently of nbldpc_amd/csrc/nbl_osd.hip: byte matrices, the eliminations step by step
// as OSD.h performs them, every candidate of the enumeration (flips of every position order[i], i < MsgLen_bit, parity positions
// included), each one re-encoded and its distance summed over ALL positions in ascending order.  The only liberty: a candidate is
// re-encoded as c0 ^ g_i ^ g_j ^ g_l (OSD_Encode_bit is linear in its input), which gives the same bits as encoding it from scratch.
// The running minimum distance is the reference's int (NBLDPC.h:127): a candidate wins when its distance is below the truncated
// distance of the last winner.  Distance and winner copy cover the first CodeLen*log(GFq)/log(2) positions, an int truncated from a
// double: 575 of the 576 bits of the BDS code, whose last bit therefore always keeps the base word's value.
// Equal reliabilities are ordered by index (a stable sort); the reference's std::sort is not stable.
//
// usage: osd_check in.bin out.bin [counters.bin]
//   in:  int32 header [N, M, q, E, order, flag, B, crc_len, crc_rows], int32 var_deg[N], var_chk[E], var_h[E] (variable-major,
//        0-based), uint8 gf_mat[q][p][p], float64 L_ch[B][N][q-1], and for flag 0: float64 S[B][N p], int32 base[B][N]
//   out: int32 out[B][N]
//   counters (optional; what the GPU tests assert their coverage on -- the decoding output does not depend on it): float64 [B][7] per
//        frame: order rotations of the elimination, pivot repairs, the largest num_temp at which a rotation happened (-1: none), the
//        flip count of the winner (0 - 3; -1: no candidate below 1,000,000, the base word stays), whether the output differs from the
//        base word, whether the winner's bit at position nd (the first one the distance leaves out) differs from the base word's
//        (0 when nd == N p or nobody won), and the smallest distance of any candidate
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

typedef std::vector<std::vector<int>> Mat;

static void g_gauss(Mat &M, int col_length, int row_length, std::vector<int> &order)
{
	for (int row = 0; row < row_length; row++) {
		int col = order[row];
		if (M[row][col] == 0) {
			bool ex = false;
			for (int up = row + 1; up < row_length; up++)
				if (M[up][col] != 0) {
					for (int i = 0; i < col_length; i++) M[row][i] ^= M[up][i];
					ex = true;
					break;
				}
			if (!ex) {
				int flag = row;
				row--;
				for (int i = flag; i < col_length - 1; i++) std::swap(order[i], order[i + 1]);
			}
		}
		for (int up = row + 1; up < row_length; up++)
			if (M[up][col] != 0)
				for (int i = 0; i < col_length; i++) M[up][i] ^= M[row][i];
	}
	for (int row = row_length - 1; row > 0; row--)
		for (int up = row - 1; up >= 0; up--)
			if (M[up][order[row]] == 1)
				for (int i = 0; i < col_length; i++) M[up][i] ^= M[row][i];
}

struct Counters { int rotations = 0, repairs = 0, max_rot = -1; };

static void h_gauss(Mat &M, int col_length, int row_length, std::vector<int> &order, Counters &cnt)
{
	for (int row = row_length - 1; row >= 0; row--) {
		int num_temp = row + col_length - row_length;
		int col = order[num_temp];
		if (M[row][col] == 0) {
			bool ex = false;
			for (int up = row - 1; up >= 0; up--)
				if (M[up][col] != 0) {
					for (int i = 0; i < col_length; i++) M[row][i] ^= M[up][i];
					ex = true;
					cnt.repairs++;
					break;
				}
			if (!ex) {
				cnt.rotations++;
				cnt.max_rot = std::max(cnt.max_rot, num_temp);
				row++;
				for (int i = num_temp - 1; i >= 0; i--) std::swap(order[i], order[i + 1]);
			}
		}
		for (int up = row - 1; up >= 0; up--)
			if (M[up][col] != 0)
				for (int i = 0; i < col_length; i++) M[up][i] ^= M[row][i];
	}
	for (int i = 0; i < row_length; i++)
		for (int j = i + 1; j < row_length; j++) {
			int pos = order[col_length - row_length + i];
			if (M[j][pos] == 1)
				for (int k = 0; k < col_length; k++) M[j][k] ^= M[i][k];
		}
}

int main(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: osd_check in.bin out.bin\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) return 2;
	int hdr[9];
	auto rd = [&](void *p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } };
	rd(hdr, sizeof hdr);
	const int N = hdr[0], M = hdr[1], q = hdr[2], E = hdr[3], order_ = hdr[4], flag = hdr[5], B = hdr[6], crcLen = hdr[7], crcRate = hdr[8];
	int p = 0;
	while ((1 << p) < q) p++;
	std::vector<int> var_deg(N), var_chk(E), var_h(E);
	rd(var_deg.data(), 4 * N); rd(var_chk.data(), 4 * E); rd(var_h.data(), 4 * E);
	std::vector<uint8_t> gm((size_t)q * p * p);
	rd(gm.data(), gm.size());
	std::vector<double> L((size_t)B * N * (q - 1));
	rd(L.data(), 8 * L.size());
	const int n = N * p, Mb = M * p, msg = n - Mb, R = crcRate + Mb;
	std::vector<double> S;
	std::vector<int> base;
	if (!flag) {
		S.resize((size_t)B * n); base.resize((size_t)B * N);
		rd(S.data(), 8 * S.size()); rd(base.data(), 4 * base.size());
	}
	fclose(f);

	// H_origin_bit (NBLDPC.cpp:409-430)
	Mat H(Mb, std::vector<int>(n, 0));
	for (int i = 0, e = 0; i < N; i++)
		for (int j = 0; j < var_deg[i]; j++, e++)
			for (int k = 0; k < p; k++)
				for (int l = 0; l < p; l++) H[p * var_chk[e] + k][p * i + l] = gm[((size_t)var_h[e] * p + l) * p + k];
	// CRCMatrixGen (OSD.h:472-509)
	Mat partH(crcRate, std::vector<int>(msg, 0));
	if (crcRate > 0) {
		Mat G(msg - crcLen, std::vector<int>(msg, 0));
		for (int i = 0; i < msg - crcLen; i++) {
			if (crcLen == 8) G[i][i] = G[i][i + 1] = G[i][i + 4] = G[i][i + 5] = G[i][i + 7] = G[i][i + 8] = 1;
			if (crcLen == 16) G[i][i] = G[i][i + 4] = G[i][i + 11] = G[i][i + 16] = 1;
			if (crcLen == 24) G[i][i] = G[i][i + 1] = G[i][i + 18] = G[i][i + 19] = G[i][i + 23] = G[i][i + 24] = 1;
		}
		std::vector<int> seri(msg);
		std::iota(seri.begin(), seri.end(), 0);
		g_gauss(G, msg, msg - crcLen, seri);
		for (int i = 0; i < crcRate; i++) {
			partH[i][i + msg - crcRate] = 1;
			for (int j = 0; j < msg - crcLen; j++) partH[i][j] = G[j][msg - crcRate + i];
		}
	}
	const int ord = order_ > 3 ? 3 : order_;
	std::vector<int> out((size_t)B * N);
	std::vector<double> counters((size_t)B * 7);
	for (int b = 0; b < B; b++) {
		const double *Lb = &L[(size_t)b * N * (q - 1)];
		std::vector<double> Lbit(n), rel(n);
		std::vector<int> base_bit(n);
		for (int i = 0; i < N; i++) {
			int a = 0;
			if (flag) {
				double mx = 0;
				for (int x = 0; x < q - 1; x++)
					if (Lb[(size_t)i * (q - 1) + x] > mx) { mx = Lb[(size_t)i * (q - 1) + x]; a = x + 1; }
			} else {
				a = base[(size_t)b * N + i];
			}
			for (int k = 0; k < p; k++) {
				Lbit[i * p + k] = Lb[(size_t)i * (q - 1) + (1 << k) - 1];
				base_bit[i * p + k] = (a >> k) & 1;
				rel[i * p + k] = std::fabs(flag ? Lbit[i * p + k] : S[(size_t)b * n + i * p + k]);
			}
		}
		std::vector<int> order(n);
		std::iota(order.begin(), order.end(), 0);
		std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return rel[a] > rel[c]; });
		Mat A(R, std::vector<int>(n, 0));
		for (int i = 0; i < crcRate; i++)
			for (int j = 0; j < msg; j++) A[i][j] = partH[i][j];
		for (int i = 0; i < Mb; i++) A[crcRate + i] = H[i];
		Counters cnt;
		h_gauss(A, n, R, order, cnt);
		const int k = n - R;
		auto encode = [&](const std::vector<int> &in, std::vector<int> &o) { // OSD_Encode_bit
			o = in;
			for (int i = 0; i < R; i++) {
				int t = 0;
				for (int j = 0; j < k; j++) t ^= A[i][order[j]] * o[order[j]];
				o[order[k + i]] = t;
			}
		};
		std::vector<int> c0;
		encode(base_bit, c0);
		std::vector<std::vector<int>> g(msg); // re-encoded flip of order[i]: zero for a parity position (the encode overwrites it)
		for (int i = 0; i < msg; i++) {
			std::vector<int> e(n, 0), o;
			e[order[i]] = 1;
			encode(e, o);
			if (i >= k) std::fill(o.begin(), o.end(), 0);
			g[i] = o;
		}
		// compute_min_distance_bit: the running minimum is an int (NBLDPC.h:127), so an accepted distance is truncated, and the
		// distance covers the first CodeLen*log(GFq)/log(2) positions, truncated too (575 of the 576 bits of the BDS code)
		int min_distance = 1000000;
		const int nd = N * std::log(q) / std::log(2);
		std::vector<int> near = base_bit, cand(n);
		int win_flips = -1, win_nd_bit = 0;
		double best = HUGE_VAL;
		auto consider = [&](int i, int j, int l) {
			for (int x = 0; x < n; x++) cand[x] = c0[x] ^ (i >= 0 ? g[i][x] : 0) ^ (j >= 0 ? g[j][x] : 0) ^ (l >= 0 ? g[l][x] : 0);
			double t = 0;
			for (int x = 0; x < nd; x++)
				if ((Lbit[x] < 0 && cand[x] == 1) || (Lbit[x] > 0 && cand[x] == 0)) t = t + std::fabs(Lbit[x]);
			best = std::min(best, t);
			if (t < min_distance) { // (the copy covers the same nd positions: the rest keep the base word's bits, OSD.h:432-436)
				win_flips = (i >= 0) + (j >= 0) + (l >= 0);
				win_nd_bit = nd < n && cand[nd] != base_bit[nd];
				min_distance = (int)t;
				std::copy(cand.begin(), cand.begin() + nd, near.begin());
			}
		};
		consider(-1, -1, -1);
		if (ord >= 1)
			for (int i = 0; i < msg; i++) consider(i, -1, -1);
		if (ord >= 2)
			for (int i = 0; i < msg; i++)
				for (int j = i + 1; j < msg; j++) consider(i, j, -1);
		if (ord >= 3)
			for (int i = 0; i < msg; i++)
				for (int j = i + 1; j < msg; j++)
					for (int l = j + 1; l < msg; l++) consider(i, j, l);
		for (int i = 0; i < N; i++) {
			int a = 0;
			for (int j = 0; j < p; j++) a = 2 * a + near[i * p + p - 1 - j];
			out[(size_t)b * N + i] = a;
		}
		double *c = &counters[(size_t)b * 7];
		c[0] = cnt.rotations; c[1] = cnt.repairs; c[2] = cnt.max_rot; c[3] = win_flips; c[4] = near != base_bit; c[5] = win_nd_bit; c[6] = best;
	}
	FILE *fo = fopen(argv[2], "wb");
	if (!fo || fwrite(out.data(), 4, out.size(), fo) != out.size()) return 2;
	fclose(fo);
	if (argc > 3) {
		FILE *fc = fopen(argv[3], "wb");
		if (!fc || fwrite(counters.data(), 8, counters.size(), fc) != counters.size()) return 2;
		fclose(fc);
	}
	return 0;
}
