// nbldpc_amd/csrc/nbl_api_create.cpp -- nbl_create and its variants: every check of the code, the field tables, the parameters and the
// layer assignment on the host, then the graph indices uploaded once (they live as long as the handle: graph_allocs).
//
// Replaces CNBLDPC::Initial's decoder set-up (NBLDPC.cpp:140-377: graph cross indices, message buffers).
// No CPU decode path exists in this library: without a HIP device nbl_create() fails.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "nbl_decoder.h"
#include "nbl_tems_path.h" // NBL_TEMS_WIDE_MAX_NC

template <typename T> static nbl_status upload(nbl_decoder *d, const std::vector<T> &h, const T **dst)
{
	void *p = nullptr;
	HIP_TRY(d, hipMalloc(&p, h.size() * sizeof(T) + 16));
	d->graph_allocs.push_back(p);
	HIP_TRY(d, hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
	*dst = (const T *)p;
	return NBL_OK;
}

static nbl_status fail_create(nbl_decoder *d, nbl_status st, const std::string &msg)
{
	g_create_error = msg.empty() && d ? d->err : msg;
	if (d) nbl_destroy(d);
	return st;
}

extern "C" nbl_status nbl_create(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv,
                                 const nbl_params *params, int device, nbl_decoder **out)
{
	return nbl_create_ex(code, gf_mul, gf_inv, params, nullptr, device, out);
}

extern "C" nbl_status nbl_create_ex(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv,
                                    const nbl_params *params, const nbl_params_ext *ext, int device, nbl_decoder **out)
{
	return nbl_create_osd(code, gf_mul, gf_inv, params, ext, nullptr, device, out);
}

// G_GaussEliminate_bit (OSD.h:258-324), literally: forward elimination with the pivot repair from the rows below and the rotation of
// order[row..] when no row has the bit
static void g_gauss_eliminate(std::vector<std::vector<uint8_t>> &m, int col_length, int row_length, std::vector<int> &order)
{
	for (int row = 0; row < row_length; row++) {
		int col = order[row];
		if (m[row][col] == 0) {
			bool exchanged = false;
			for (int up = row + 1; up < row_length; up++)
				if (m[up][col] != 0) {
					for (int i = 0; i < col_length; i++) m[row][i] ^= m[up][i];
					exchanged = true;
					break;
				}
			if (!exchanged) {
				const int flag = row;
				row--;
				for (int i = flag; i < col_length - 1; i++) std::swap(order[i], order[i + 1]);
			}
		}
		for (int up = row + 1; up < row_length; up++)
			if (m[up][col] != 0)
				for (int i = 0; i < col_length; i++) m[up][i] ^= m[row][i];
	}
	for (int row = row_length - 1; row > 0; row--)
		for (int up = row - 1; up >= 0; up--)
			if (m[up][order[row]] == 1)
				for (int i = 0; i < col_length; i++) m[up][i] ^= m[row][i];
}

// [CRC rows; H_bit] of Decoding_OSD_bit (OSD.h:44-57): H_bit as CNBLDPC::Initial builds it (NBLDPC.cpp:416-430, plain assignment in
// variable-major edge order), the CRC rows as CRCMatrixGen (OSD.h:472-509).  Returns the rows, or an error text.
static std::string osd_matrix(const nbl_code_desc *code, int p, const nbl_osd_params *o, std::vector<std::vector<uint8_t>> &rows)
{
	const int N = code->N, M = code->M, n = N * p, Mb = M * p, msg = n - Mb, L = o->crc_len, cr = o->crc_rows;
	std::vector<std::vector<uint8_t>> H((size_t)Mb, std::vector<uint8_t>(n, 0));
	for (int v = 0, e = 0; v < N; v++)
		for (int j = 0; j < code->var_deg[v]; j++, e++) {
			const int chk = code->var_chk[e], h = code->var_h[e];
			for (int k = 0; k < p; k++)
				for (int l = 0; l < p; l++) H[(size_t)p * chk + k][(size_t)p * v + l] = o->gf_mat[((size_t)h * p + l) * p + k];
		}
	rows.clear();
	if (cr > 0) {
		if (msg - L <= 0) return "OSD: the CRC generator has no rows (crc_len >= N p - M p)";
		std::vector<std::vector<uint8_t>> G((size_t)(msg - L), std::vector<uint8_t>(msg, 0));
		static const int taps8[] = {0, 1, 4, 5, 7, 8}, taps16[] = {0, 4, 11, 16}, taps24[] = {0, 1, 18, 19, 23, 24};
		const int *taps = L == 8 ? taps8 : L == 16 ? taps16 : taps24;
		const int ntaps = L == 16 ? 4 : 6;
		for (int i = 0; i < msg - L; i++)
			for (int t = 0; t < ntaps; t++) G[i][i + taps[t]] = 1;
		std::vector<int> seri(msg);
		for (int i = 0; i < msg; i++) seri[i] = i;
		g_gauss_eliminate(G, msg, msg - L, seri);
		for (int i = 0; i < cr; i++) {
			std::vector<uint8_t> r(n, 0);
			r[i + msg - cr] = 1;
			for (int j = 0; j < msg - L; j++) r[j] = G[j][msg - cr + i];
			rows.push_back(r);
		}
	}
	for (auto &r : H) rows.push_back(r);
	return "";
}

// GF(2) rank of a row set (column order does not matter)
static int gf2_rank(std::vector<std::vector<uint64_t>> m, int nw)
{
	int rank = 0;
	const int R = (int)m.size();
	for (int c = 0; c < nw * 64 && rank < R; c++) {
		int piv = -1;
		for (int r = rank; r < R; r++)
			if ((m[r][c >> 6] >> (c & 63)) & 1) { piv = r; break; }
		if (piv < 0) continue;
		std::swap(m[piv], m[rank]);
		for (int r = 0; r < R; r++)
			if (r != rank && ((m[r][c >> 6] >> (c & 63)) & 1))
				for (int x = 0; x < nw; x++) m[r][x] ^= m[rank][x];
		rank++;
	}
	return rank;
}

// The caller's field tables, checked in full before anything is indexed by one of their entries: gf_mul must be THE table of
// GF(2)[x] / poly in the polynomial basis (poly read off x * x^(p-1)), gf_inv its inverses.  Some kernels multiply by shift and
// XOR with poly, others look gf_mul up as bytes or through offsets built from it: they decode the same code only if the whole
// table is that product.  Every non-zero element has an inverse exactly when poly is irreducible, so a reducible modulus is
// refused by the last condition.  Returns poly, or 0 with the first offending entry named in `msg`.
static int validate_field(int q, const uint16_t *gf_mul, const uint16_t *gf_inv, std::string &msg)
{
	const int p = ilog2(q);
	for (int a = 0; a < q; a++)
		for (int b = 0; b < q; b++)
			if (gf_mul[(size_t)a * q + b] >= q) {
				msg = "gf_mul[" + std::to_string(a) + "][" + std::to_string(b) + "] = " + std::to_string(gf_mul[(size_t)a * q + b]) + " is not an element of GF(" + std::to_string(q) + ")";
				return 0;
			}
	for (int a = 0; a < q; a++)
		if (gf_mul[a] != 0 || gf_mul[(size_t)a * q] != 0) {
			const bool row = gf_mul[a] != 0;
			msg = "gf_mul[" + std::to_string(row ? 0 : a) + "][" + std::to_string(row ? a : 0) + "] is not zero";
			return 0;
		}
	// x * x^(p-1) = x^p = poly - q
	const int poly = q | gf_mul[(size_t)2 * q + (q >> 1)];
	for (int a = 1; a < q; a++)
		for (int b = 1; b < q; b++) {
			int acc = 0, x = a;
			for (int i = 0; i < p; i++) {
				if ((b >> i) & 1) acc ^= x;
				x <<= 1;
				if (x & q) x ^= poly;
			}
			if (gf_mul[(size_t)a * q + b] != acc) {
				msg = "gf_mul is not a polynomial-basis GF(2^p) table: gf_mul[" + std::to_string(a) + "][" + std::to_string(b) + "] = " + std::to_string(gf_mul[(size_t)a * q + b]) +
				      ", the product modulo " + std::to_string(poly) + " is " + std::to_string(acc);
				return 0;
			}
		}
	for (int a = 1; a < q; a++) {
		if (gf_inv[a] >= q) {
			msg = "gf_inv[" + std::to_string(a) + "] = " + std::to_string(gf_inv[a]) + " is not an element of GF(" + std::to_string(q) + ")";
			return 0;
		}
		if (gf_mul[(size_t)a * q + gf_inv[a]] != 1) {
			msg = "gf_inv inconsistent with gf_mul: gf_mul[" + std::to_string(a) + "][gf_inv[" + std::to_string(a) + "] = " + std::to_string(gf_inv[a]) + "] is not 1 (modulus " +
			      std::to_string(poly) + "; a reducible modulus has elements without an inverse)";
			return 0;
		}
	}
	return poly;
}

// ---- layer assignments of the layered schedule (include/nbldpc.h): pure host arithmetic --------------------------------------
// Greedy colouring on a checked graph: checks in ascending index, each gets the smallest layer that holds no check sharing a
// variable with it.  Returns the number of layers.
static int layer_greedy(int N, int M, const std::vector<int> &coff, const int32_t *chk_var, int32_t *layer_of)
{
	std::vector<std::vector<int>> used(N);  // layers of the checks each variable has joined so far
	std::vector<int> stamp(M + 1, -1);
	int n_layers = 0;
	for (int m = 0; m < M; m++) {
		for (int ce = coff[m]; ce < coff[m + 1]; ce++)
			for (int l : used[chk_var[ce]]) stamp[l] = m;
		int l = 0;
		while (stamp[l] == m) l++; // (at most M - 1 layers are taken: stamp[M] is never reached)
		layer_of[m] = l;
		if (l + 1 > n_layers) n_layers = l + 1;
		for (int ce = coff[m]; ce < coff[m + 1]; ce++) {
			std::vector<int> &u = used[chk_var[ce]];
			bool have = false;
			for (int x : u) have = have || x == l;
			if (!have) u.push_back(l);
		}
	}
	return n_layers;
}

// A caller's assignment: every index >= 0, every layer up to the largest index used non-empty, no two checks of a layer sharing a
// variable.  Returns the number of layers, or 0 with the offence named in `msg`.
static int layer_validate(int N, int M, const std::vector<int> &coff, const int32_t *chk_var, const int32_t *layer_of, std::string &msg)
{
	int n_layers = 0;
	for (int m = 0; m < M; m++) {
		if (layer_of[m] < 0) { msg = "layered schedule: layer_of[" + std::to_string(m) + "] = " + std::to_string(layer_of[m]) + " is below 0"; return 0; }
		if (layer_of[m] >= M) { msg = "layered schedule: layer " + std::to_string(layer_of[m]) + " of check " + std::to_string(m) + " leaves an empty layer below it (M = " + std::to_string(M) + " checks)"; return 0; }
		if (layer_of[m] + 1 > n_layers) n_layers = layer_of[m] + 1;
	}
	std::vector<int> count(n_layers, 0);
	for (int m = 0; m < M; m++) count[layer_of[m]]++;
	for (int l = 0; l < n_layers; l++)
		if (!count[l]) { msg = "layered schedule: layer " + std::to_string(l) + " is empty (the largest layer index used is " + std::to_string(n_layers - 1) + ")"; return 0; }
	// per variable: the check that claimed each layer first
	std::vector<std::vector<std::pair<int, int>>> seen(N);
	for (int m = 0; m < M; m++)
		for (int ce = coff[m]; ce < coff[m + 1]; ce++) {
			const int n = chk_var[ce];
			for (const auto &pr : seen[n])
				if (pr.first == layer_of[m] && pr.second != m) {
					msg = "layered schedule: checks " + std::to_string(pr.second) + " and " + std::to_string(m) + " of layer " + std::to_string(layer_of[m]) + " share variable " + std::to_string(n);
					return 0;
				}
			seen[n].push_back({layer_of[m], m});
		}
	return n_layers;
}

extern "C" int32_t nbl_layer_greedy(const nbl_code_desc *code, int32_t *layer_of)
{
	if (!code || !layer_of || !code->chk_deg || !code->chk_var) { g_create_error = "null argument"; return NBL_ERR_ARG; }
	const int N = code->N, M = code->M;
	if (N <= 0 || M <= 0) { g_create_error = "N, M must be positive"; return NBL_ERR_ARG; }
	std::vector<int> coff(M + 1, 0);
	for (int m = 0; m < M; m++) {
		if (code->chk_deg[m] < 1 || code->chk_deg[m] > N) { g_create_error = "check degree out of range"; return NBL_ERR_ARG; }
		coff[m + 1] = coff[m] + code->chk_deg[m];
	}
	for (int ce = 0; ce < coff[M]; ce++)
		if (code->chk_var[ce] < 0 || code->chk_var[ce] >= N) { g_create_error = "check-side edge out of range"; return NBL_ERR_ARG; }
	return layer_greedy(N, M, coff, code->chk_var, layer_of);
}

// nbl_create_layered's / nbl_create_layered_ex's / nbl_create_layered_bp's request: layer_of == NULL asks for the greedy assignment;
// flags: NBL_LAYERED_*; bp: the log-QSPA entry point (method 1 alone, its own damping: no flag)
struct LayerReq { const int32_t *layer_of; uint32_t flags; bool bp; };

static nbl_status create_impl(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                              const nbl_params_ext *ext, const nbl_osd_params *osd, const LayerReq *lay, int device, nbl_decoder **out,
                              NblKind kind);

extern "C" nbl_status nbl_create_osd(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                     const nbl_params_ext *ext, const nbl_osd_params *osd, int device, nbl_decoder **out)
{
	return create_impl(code, gf_mul, gf_inv, params, ext, osd, nullptr, device, out, NBL_KIND_BASE);
}

extern "C" nbl_status nbl_create_layered(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                         const int32_t *layer_of, int device, nbl_decoder **out)
{
	const LayerReq lay = {layer_of, 0, false};
	return create_impl(code, gf_mul, gf_inv, params, nullptr, nullptr, &lay, device, out, NBL_KIND_BASE);
}

extern "C" nbl_status nbl_create_layered_ex(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                            const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	const LayerReq lay = {layer_of, flags, false};
	return create_impl(code, gf_mul, gf_inv, params, nullptr, nullptr, &lay, device, out, NBL_KIND_BASE);
}

extern "C" nbl_status nbl_create_layered_bp(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                            const int32_t *layer_of, int device, nbl_decoder **out)
{
	const LayerReq lay = {layer_of, 0, true};
	return create_impl(code, gf_mul, gf_inv, params, nullptr, nullptr, &lay, device, out, NBL_KIND_BASE);
}

// The entry points that name a kind (include/nbldpc.h).  Each is flooding without a LayerReq and layered with the request of the
// nbl_create_layered* function its row names -- the same assignment rules, the same v2c state (EMS: none)
#define NBL_STR_(x) #x
#define NBL_STR(x) NBL_STR_(x)
static constexpr const char *FHT_ONLY = " runs the sum-product rule of log-QSPA (method 1) only: the transform evaluates its XOR convolution, which no other "
                                        "method's check node is";
static const NblEntry nbl_entries[] = {
	// FHT sum-product decoding.  The wide programme's storage does not grow with the check degree, so its limit is the LDS block's, 32; the
	// variable side -- the layer rows, the variable-node pass -- keeps 8 everywhere.  Layered: nbl_create_layered_bp
	{NBL_KIND_FHT, "fht", "nbl_create_fht", NBL_FHT_LAYERED, "NBL_FHT_LAYERED", NBL_METHOD_BP, FHT_ONLY, NBL_FHT_MAX_CHECK_DEGREE, "", 0, true},
	// The same in single precision: a float message state.  The product of up to 7 transformed vectors and its transform stay inside
	// binary32's range; no wide layout
	{NBL_KIND_FHT32, "fht32", "nbl_create_fht32", NBL_FHT32_LAYERED, "NBL_FHT32_LAYERED", NBL_METHOD_BP, FHT_ONLY, NBL_MAXDC,
	 ": products of more transformed vectors leave the range of single precision; nbl_create_fht (double precision) takes check degrees up to "
	 NBL_STR(NBL_FHT_MAX_CHECK_DEGREE), 0, true},
	// Single precision above degree 8: every transformed input is scaled by a power of two (step 3a), which keeps the products in range; the
	// wide layout's limit is the LDS block's, 32.  maxdc q 4 bytes, at most 32 KB -- nothing to refuse for LDS.  Layered: nbl_create_layered_bp
	{NBL_KIND_FHT32_WIDE, "fht32_wide", "nbl_create_fht32_wide", NBL_FHT32_WIDE_LAYERED, "NBL_FHT32_WIDE_LAYERED", NBL_METHOD_BP, FHT_ONLY,
	 NBL_FHT32_MAX_CHECK_DEGREE, "", 0, true},
	// EMS, one workgroup per check, no array sized by the degree; the limit is the header's, the LDS bound is checked in create_impl.
	// Layered: nbl_create_layered
	{NBL_KIND_EMS_WIDE, "ems_wide", "nbl_create_ems_wide", NBL_EMS_WIDE_LAYERED, "NBL_EMS_WIDE_LAYERED", NBL_METHOD_EMS,
	 " runs EMS (method 2) only: the other methods keep their entry points and their check-degree limit of 8 (log-QSPA above it: nbl_create_fht)",
	 NBL_EMS_MAX_CHECK_DEGREE, "", 0, false},
	// T-EMS over any field, the same shape of programme; its path code holds columns up to 31.  Layered: nbl_create_layered_ex(..,
	// NBL_LAYERED_DAMPED)
	{NBL_KIND_TEMS_WIDE, "tems_wide", "nbl_create_tems_wide", NBL_TEMS_WIDE_LAYERED, "NBL_TEMS_WIDE_LAYERED", NBL_METHOD_TEMS,
	 " runs T-EMS (method 4) only: the other methods keep their entry points (EMS above check degree 8: nbl_create_ems_wide, log-QSPA: nbl_create_fht)",
	 NBL_TEMS_MAX_CHECK_DEGREE, "", NBL_LAYERED_DAMPED, false},
	// Exact log-QSPA, the same shape of programme; (maxdc + 5) q 8 + 256 bytes of LDS, at most 76,032 B -- nothing to refuse for LDS.
	// Layered: nbl_create_layered_bp
	{NBL_KIND_BP_WIDE, "bp_wide", "nbl_create_bp_wide", NBL_BP_WIDE_LAYERED, "NBL_BP_WIDE_LAYERED", NBL_METHOD_BP,
	 " runs exact log-QSPA (method 1) only: the other methods keep their entry points (EMS above check degree 8: nbl_create_ems_wide, T-EMS: nbl_create_tems_wide)",
	 NBL_BP_MAX_CHECK_DEGREE, "", 0, true},
	// Min-Max, the same shape of programme; (maxdc + 4) q 8 bytes of LDS, at most 73,728 B -- nothing to refuse for LDS.  Layered:
	// nbl_create_layered
	{NBL_KIND_MINMAX, "minmax", "nbl_create_minmax", NBL_MINMAX_LAYERED, "NBL_MINMAX_LAYERED", NBL_METHOD_MINMAX,
	 " runs Min-Max (method 3) only: the other methods keep their entry points (EMS: nbl_create / nbl_create_ems_wide, T-EMS: nbl_create_tems_wide, log-QSPA: "
	 "nbl_create_bp_wide / nbl_create_fht)",
	 NBL_MINMAX_MAX_CHECK_DEGREE, "", 0, false},
};

const NblEntry *nbl_entry(NblKind kind)
{
	for (const NblEntry &en : nbl_entries)
		if (en.kind == kind) return &en;
	return nullptr;
}

const NblEntry *nbl_entry_named(const char *name)
{
	for (const NblEntry &en : nbl_entries)
		if (name && !strcmp(en.name, name)) return &en;
	return nullptr;
}

static nbl_status create_kind(NblKind kind, const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                              const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	const NblEntry &en = *nbl_entry(kind);
	if (!out) return NBL_ERR_ARG;
	*out = nullptr;
	if (flags & ~en.layered_bit)
		return fail_create(nullptr, NBL_ERR_ARG, std::string(en.fn) + ": unknown flag bit (flags = " + std::to_string(flags) + "; " + en.layered_flag + " = " +
		                                         std::to_string(en.layered_bit) + " is the only one defined)");
	if (!(flags & en.layered_bit) && layer_of)
		return fail_create(nullptr, NBL_ERR_ARG, std::string(en.fn) + ": a layer assignment belongs to the layered schedule (flags = 0 is flooding: pass layer_of = NULL, or set " +
		                                         en.layered_flag + ")");
	const LayerReq lay = {layer_of, en.lay_flags, en.lay_bp};
	return create_impl(code, gf_mul, gf_inv, params, nullptr, nullptr, (flags & en.layered_bit) ? &lay : nullptr, device, out, kind);
}

extern "C" nbl_status nbl_create_fht(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                     const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	return create_kind(NBL_KIND_FHT, code, gf_mul, gf_inv, params, layer_of, flags, device, out);
}

extern "C" nbl_status nbl_create_fht32(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                       const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	return create_kind(NBL_KIND_FHT32, code, gf_mul, gf_inv, params, layer_of, flags, device, out);
}

extern "C" nbl_status nbl_create_fht32_wide(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                            const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	return create_kind(NBL_KIND_FHT32_WIDE, code, gf_mul, gf_inv, params, layer_of, flags, device, out);
}

extern "C" nbl_status nbl_create_ems_wide(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                          const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	return create_kind(NBL_KIND_EMS_WIDE, code, gf_mul, gf_inv, params, layer_of, flags, device, out);
}

extern "C" nbl_status nbl_create_tems_wide(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                           const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	return create_kind(NBL_KIND_TEMS_WIDE, code, gf_mul, gf_inv, params, layer_of, flags, device, out);
}

extern "C" nbl_status nbl_create_bp_wide(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                         const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	return create_kind(NBL_KIND_BP_WIDE, code, gf_mul, gf_inv, params, layer_of, flags, device, out);
}

extern "C" nbl_status nbl_create_minmax(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                                        const int32_t *layer_of, uint32_t flags, int device, nbl_decoder **out)
{
	return create_kind(NBL_KIND_MINMAX, code, gf_mul, gf_inv, params, layer_of, flags, device, out);
}

extern "C" nbl_status nbl_get_layers(const nbl_decoder *d, int32_t *layer_of, int32_t *n_layers)
{
	if (!d || !d->layered) return NBL_ERR_ARG;
	if (layer_of) memcpy(layer_of, d->h_layer_of.data(), d->h_layer_of.size() * sizeof(int32_t));
	if (n_layers) *n_layers = d->n_layers;
	return NBL_OK;
}

static nbl_status create_impl(const nbl_code_desc *code, const uint16_t *gf_mul, const uint16_t *gf_inv, const nbl_params *params,
                              const nbl_params_ext *ext, const nbl_osd_params *osd, const LayerReq *lay, int device, nbl_decoder **out, NblKind kind)
{
	const NblEntry *const en = nbl_entry(kind); // NULL: nbl_create* / nbl_create_layered*
	const bool ems_wide = kind == NBL_KIND_EMS_WIDE, tems_wide = kind == NBL_KIND_TEMS_WIDE;
	const bool minmax = kind == NBL_KIND_MINMAX; // (method 3 has passed the entry's own method check below: its schedule is that of EMS)
	if (!out) return NBL_ERR_ARG;
	*out = nullptr;
	if (!code || !gf_mul || !gf_inv || !params) return fail_create(nullptr, NBL_ERR_ARG, "null argument");
	if (lay && (lay->flags & ~(uint32_t)NBL_LAYERED_DAMPED))
		return fail_create(nullptr, NBL_ERR_ARG, "layered schedule: unknown flag bit (flags = " + std::to_string(lay->flags) + "; NBL_LAYERED_DAMPED = 1 is the only one defined)");
	const int N = code->N, M = code->M, q = code->q;
	if (N <= 0 || M <= 0 || q < 4 || (q & (q - 1))) return fail_create(nullptr, NBL_ERR_ARG, "N, M must be positive and q a power of two, at least 4");
	// (the reference ships arithmetic tables up to GF(512) but no code above GF(256); a valid request this library cannot serve)
	if (q > 256) return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "fields above GF(256) are not supported (one wave holds at most 4 symbols per lane)");
	std::string field_err;
	const int poly = validate_field(q, gf_mul, gf_inv, field_err);
	if (!poly) return fail_create(nullptr, NBL_ERR_ARG, field_err);
	if (en && params->method != en->method) return fail_create(nullptr, NBL_ERR_UNSUPPORTED, std::string(en->fn) + en->method_text);
	if (lay && lay->bp && params->method != NBL_METHOD_BP)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "nbl_create_layered_bp runs log-QSPA (method 1) only: the layered schedule of EMS (method 2) is behind "
		                                                 "nbl_create_layered, that of T-EMS (method 4) behind nbl_create_layered_ex with NBL_LAYERED_DAMPED");
	if (lay && !lay->bp && (lay->flags & NBL_LAYERED_DAMPED) && params->method != NBL_METHOD_EMS && params->method != NBL_METHOD_TEMS)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "the damped layered schedule (NBL_LAYERED_DAMPED) is defined for T-EMS (method 4), and for EMS (method 2), which "
		                                                 "has no damping, as the plain layered schedule: log-QSPA (method 1) and BS-TEMS (method 7) stay flooding-only");
	if (lay && !lay->bp && !minmax && params->method != NBL_METHOD_EMS && !((lay->flags & NBL_LAYERED_DAMPED) && params->method == NBL_METHOD_TEMS))
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "the layered schedule is defined for EMS (method 2) only: the other methods damp against the previous iteration's "
		                                                 "decision in their variable-node pass and stay flooding-only");
	// (method 3 through nbl_create_minmax alone: every other entry point takes the default's refusal, as before)
	switch (minmax ? NBL_METHOD_EMS : params->method) {
	case NBL_METHOD_EMS: case NBL_METHOD_BP: case NBL_METHOD_TEMS: break;
	case NBL_METHOD_BS_TEMS:
		if (!ext) return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "BS-TEMS (method 7): its parameters (bs_nm, bs_nc, bs_factor, bs_offset) go through nbl_create_ex");
		break;
	case NBL_METHOD_OSD:
		if (!osd) return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "OSD (method 6): its parameters (order, flag, factor, crc_len, crc_rows, gf_mat) go through nbl_create_osd");
		break;
	default: return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "decode method not supported (reference: 'has not been developed')");
	}
	// ---- OSD parameters and the binary matrix, before any device call ----
	const bool osd_on = osd && (params->method == NBL_METHOD_OSD || osd->order >= 0);
	std::vector<uint64_t> osd_words;
	int osd_R = 0;
	if (osd) {
		if (osd->order < -1) return fail_create(nullptr, NBL_ERR_ARG, "OSD: order < -1");
		if (osd->flag != 0 && osd->flag != 1) return fail_create(nullptr, NBL_ERR_ARG, "OSD: flag must be 0 or 1");
		if (!osd->gf_mat) return fail_create(nullptr, NBL_ERR_ARG, "OSD: gf_mat is NULL");
		for (int p1 = ilog2(q), i = 0; i < p1 * p1; i++) // the matrix of "multiply by 1"
			if (osd->gf_mat[(size_t)p1 * p1 + i] != (i / p1 == i % p1))
				return fail_create(nullptr, NBL_ERR_ARG, "OSD: gf_mat of element 1 is not the identity (entry [" + std::to_string(i / p1) + "][" + std::to_string(i % p1) + "])");
		if (osd->crc_rows < 0 || osd->crc_rows > osd->crc_len) return fail_create(nullptr, NBL_ERR_ARG, "OSD: crc_rows must be in 0 .. crc_len");
		if (osd->crc_rows > 0 && osd->crc_len != 8 && osd->crc_len != 16 && osd->crc_len != 24)
			return fail_create(nullptr, NBL_ERR_ARG, "OSD: CRC rows need crc_len 8, 16 or 24 (the reference's CRC generator is empty otherwise and its elimination never ends)");
	}
	if (osd_on) {
		const int p = ilog2(q), n = N * p;
		// (every n up to the cap fits: nbl_osd_lds_bytes(1024, .) = 160,464 B of the 163,840 B of one workgroup; checked here, before any
		// device call, so that a change of either limit cannot reach the first decode)
		if (n > NBL_OSD_MAX_BITS || nbl_osd_lds_bytes(n, 0) > NBL_OSD_MAX_LDS)
			return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "OSD: N log2(q) above NBL_OSD_MAX_BITS (1024) does not fit the kernel's LDS");
		for (int v = 0, e = 0; v < N; v++) // (the graph is validated below; the matrix build must not index outside it first)
			for (int j = 0; j < code->var_deg[v]; j++, e++)
				if (code->var_deg[v] < 1 || code->var_chk[e] < 0 || code->var_chk[e] >= M || code->var_h[e] <= 0 || code->var_h[e] >= q)
					return fail_create(nullptr, NBL_ERR_ARG, "variable-side edge out of range");
		std::vector<std::vector<uint8_t>> rows;
		const std::string e = osd_matrix(code, p, osd, rows);
		if (!e.empty()) return fail_create(nullptr, NBL_ERR_ARG, e);
		osd_R = (int)rows.size();
		if (osd_R >= n) return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "OSD: the matrix has no fewer rows than columns");
		const int nw = (n + 63) / 64;
		std::vector<std::vector<uint64_t>> packed(osd_R, std::vector<uint64_t>(nw, 0));
		for (int r = 0; r < osd_R; r++)
			for (int c = 0; c < n; c++)
				if (rows[r][c]) packed[r][c >> 6] |= 1ull << (c & 63);
		if (gf2_rank(packed, nw) != osd_R)
			return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "OSD: [CRC rows; H_bit] is not of full row rank (the reference's elimination never ends on it)");
		for (auto &r : packed) osd_words.insert(osd_words.end(), r.begin(), r.end());
	}
	if (params->max_iter < 0) return fail_create(nullptr, NBL_ERR_ARG, "max_iter < 0");
	if (params->method == NBL_METHOD_EMS) {
		// reference: "EMS configuration error! EMS_Nm is too large!" + exit(-1), NBLDPC.cpp:282-286
		if (params->ems_nm > q) return fail_create(nullptr, NBL_ERR_ARG, "EMS configuration error! EMS_Nm is too large!");
		if (params->ems_nm < 1 || params->ems_nc < 0) return fail_create(nullptr, NBL_ERR_ARG, "ems_nm < 1 or ems_nc < 0");
	}
	// (Min-Max reads its shaping from the EMS fields; nm and nc are not read)
	if (minmax && !(params->ems_factor != 0.0)) return fail_create(nullptr, NBL_ERR_ARG, "nbl_create_minmax: ems_factor must be non-zero (c2v values are divided by it)");
	if (params->method == NBL_METHOD_TEMS && (params->tems_nr < 1 || params->tems_nc < 0))
		return fail_create(nullptr, NBL_ERR_ARG, "tems_nr < 1 or tems_nc < 0");
	if (params->method == NBL_METHOD_BS_TEMS) {
		// the reference's basic-set arrays hold q elements (NBLDPC.cpp:333): bs_nm >= q reads past them
		if (ext->bs_nm < 1 || ext->bs_nm >= q) return fail_create(nullptr, NBL_ERR_ARG, "BS-TEMS: bs_nm must be at least 1 and below q");
		if (ext->bs_nc < 0) return fail_create(nullptr, NBL_ERR_ARG, "BS-TEMS: bs_nc < 0");
		if (!(ext->bs_factor != 0.0)) return fail_create(nullptr, NBL_ERR_ARG, "BS-TEMS: bs_factor must be non-zero (c2v values are divided by it)");
		if (ext->bs_nm > 16)
			return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "BS-TEMS: bs_nm above 16 is not supported (the kernel enumerates configurations as bs_nm-bit masks)");
	}

	// ---- host-side graph indices (NBLDPC.cpp:236-263) -------------------------------------------------------
	std::vector<int> voff(N + 1, 0), coff(M + 1, 0);
	const NblShape shape = nbl_shape(code);
	const int maxdv = shape.maxdv, maxdc = shape.maxdc, p = shape.p;
	for (int n = 0; n < N; n++) {
		if (code->var_deg[n] < 1) return fail_create(nullptr, NBL_ERR_ARG, "variable of degree < 1");
		voff[n + 1] = voff[n] + code->var_deg[n];
	}
	for (int m = 0; m < M; m++) {
		if (code->chk_deg[m] < 2) return fail_create(nullptr, NBL_ERR_ARG, "check of degree < 2");
		coff[m + 1] = coff[m] + code->chk_deg[m];
	}
	const int E = voff[N];
	if (coff[M] != E) return fail_create(nullptr, NBL_ERR_ARG, "variable-side and check-side edge counts differ");
	// (a kind's own check-degree ceiling, with its own text, where the variable side is in range: that side keeps 8 everywhere)
	if (en && maxdv <= NBL_MAXDV && maxdc > en->max_dc)
		return fail_create(nullptr, NBL_ERR_ARG, std::string(en->fn) + ": check degree " + std::to_string(maxdc) + " above the supported maximum (" +
		                                         std::to_string(en->max_dc) + ")" + en->max_dc_text);
	if ((kind == NBL_KIND_BASE && maxdc > NBL_MAXDC) || maxdv > NBL_MAXDV) return fail_create(nullptr, NBL_ERR_ARG, "node degree above the supported maximum (8)");
	static_assert(NBL_LAYER_ROW >= 4 + NBL_MAXDV, "a layer row holds the c2v slots of every edge of a variable");
	std::vector<int> v_cpos(E, -1), c_epos(E, -1), c_var(E), c_h(E), c_hinv(E);
	for (int ce = 0; ce < E; ce++) {
		int n = code->chk_var[ce], h = code->chk_h[ce];
		if (n < 0 || n >= N || h <= 0 || h >= q) return fail_create(nullptr, NBL_ERR_ARG, "check-side edge out of range / zero coefficient");
		c_var[ce] = n;
		c_h[ce] = h;
		c_hinv[ce] = gf_inv[h];
	}
	for (int n = 0; n < N; n++)
		for (int e = voff[n]; e < voff[n + 1]; e++) {
			int m = code->var_chk[e];
			if (m < 0 || m >= M) return fail_create(nullptr, NBL_ERR_ARG, "variable-side edge out of range");
			for (int ce = coff[m]; ce < coff[m + 1]; ce++)
				if (c_var[ce] == n) v_cpos[e] = ce; // last match wins, like VarLinkDc
			if (v_cpos[e] < 0 || c_h[v_cpos[e]] != code->var_h[e]) return fail_create(nullptr, NBL_ERR_ARG, "variable-side and check-side edge lists disagree");
		}
	for (int m = 0; m < M; m++)
		for (int ce = coff[m]; ce < coff[m + 1]; ce++) {
			int n = c_var[ce];
			for (int e = voff[n]; e < voff[n + 1]; e++)
				if (code->var_chk[e] == m) c_epos[ce] = e; // like ChkLinkDv
			if (c_epos[ce] < 0) return fail_create(nullptr, NBL_ERR_ARG, "check-side edge without variable-side partner");
		}
	// shape limits of the kernels, refused here rather than at the first decode
	// (nbl_create_tems_wide: such a code runs the programme whose path code does not grow with the degree, nbl_tems_path.h)
	const bool tems_needs_wide = tems_wide && nbl_tems_needs_wide(shape);
	if (params->method == NBL_METHOD_TEMS && !tems_wide && p * maxdc > 32)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "T-EMS: log2(q) * (largest check degree) must not exceed 32 (the trellis path code is one 32-bit word)");
	// (a wide decoder with maxdc <= NBL_MAXDC may run either programme: both bounds hold, the general kernel's first, with nbl_create's text)
	if (params->method == NBL_METHOD_EMS && !(ems_wide && maxdc > NBL_MAXDC) && nbl_ems_lds_bytes(q, maxdc, params->ems_nm, params->ems_nc) > NBL_MAX_LDS)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "EMS: this (q, check degree, nm, nc) needs more than the 160 KB of LDS one wave can have");
	if (ems_wide && nbl_ems_wide_lds_bytes(q, maxdc, params->ems_nm, params->ems_nc) > NBL_MAX_LDS)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "nbl_create_ems_wide: this (q, check degree, nm, nc) needs " +
		                                                 std::to_string(nbl_ems_wide_lds_bytes(q, maxdc, params->ems_nm, params->ems_nc)) +
		                                                 " bytes of LDS per check, more than the 160 KB (163840 bytes) one workgroup can have");
	if (tems_needs_wide && params->tems_nc > NBL_TEMS_WIDE_MAX_NC)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "nbl_create_tems_wide: tems_nc = " + std::to_string(params->tems_nc) + " above " + std::to_string(NBL_TEMS_WIDE_MAX_NC) +
		                                                 " (NBL_TEMS_WIDE_MAX_NC: the deviations one 64-bit path code holds) on a code whose checks need the wide programme");
	// (inside nbl_create's envelope the bound holds wherever switch 3 may select the wide programme; it is far from it there)
	if (tems_wide && params->tems_nc <= NBL_TEMS_WIDE_MAX_NC && nbl_tems_wide_lds_bytes(q, maxdc, params->tems_nr, params->tems_nc) > NBL_MAX_LDS)
		return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "nbl_create_tems_wide: this (q, check degree, nr, nc) needs " +
		                                                 std::to_string(nbl_tems_wide_lds_bytes(q, maxdc, params->tems_nr, params->tems_nc)) +
		                                                 " bytes of LDS per check, more than the 160 KB (163840 bytes) one workgroup can have");
	// ---- layered schedule: the assignment, checked or made here, before the device is touched ----
	std::vector<int> layer_of, lay_off, lay_chk, lay_nbr;
	int n_layers = 0;
	if (lay) {
		// (the layered kernel is the general one: no specialised shape stands in for it, so the LDS bound holds for every shape)
		// (log-QSPA: (3 maxdc + 5) q 8 bytes, at most 59,392 B at q = 256 and degree 8, the largest check every entry point but
		// nbl_create_bp_wide accepts -- nothing to refuse; above degree 8 nbl_create_bp_wide runs the workgroup-per-check programme alone,
		// (maxdc + 5) q 8 + 256 bytes, at most 76,032 B at q = 256 and degree 32 (nbl_bp_wide_lds_bytes), which its launchers opt in for --
		// nothing to refuse either; FHT: maxdc q 8 bytes, at most
		// 65,536 B at q = 256 and degree 32, what a launch gets without opting in -- nothing to refuse either; in single precision
		// maxdc q 4 bytes, half of that)
		if (params->method == NBL_METHOD_TEMS) {
			if (!tems_needs_wide && nbl_tems_layered_lds_bytes(q, maxdc, params->tems_nc) > NBL_MAX_LDS)
				return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "T-EMS: this (q, check degree, nc) needs more than the 160 KB of LDS one wave can have");
		} else if (params->method == NBL_METHOD_EMS && !(ems_wide && maxdc > NBL_MAXDC) && nbl_ems_lds_bytes(q, maxdc, params->ems_nm, params->ems_nc) > NBL_MAX_LDS) {
			return fail_create(nullptr, NBL_ERR_UNSUPPORTED, "EMS: this (q, check degree, nm, nc) needs more than the 160 KB of LDS one wave can have");
		}
		layer_of.assign(M, 0);
		if (lay->layer_of) {
			std::string lerr;
			n_layers = layer_validate(N, M, coff, code->chk_var, lay->layer_of, lerr);
			if (!n_layers) return fail_create(nullptr, NBL_ERR_ARG, lerr);
			layer_of.assign(lay->layer_of, lay->layer_of + M);
		} else {
			n_layers = layer_greedy(N, M, coff, code->chk_var, layer_of.data());
		}
		lay_off.assign(n_layers + 1, 0);
		for (int m = 0; m < M; m++) lay_off[layer_of[m] + 1]++;
		for (int l = 0; l < n_layers; l++) lay_off[l + 1] += lay_off[l];
		lay_chk.assign(M, 0);
		std::vector<int> fill(lay_off.begin(), lay_off.end() - 1);
		for (int m = 0; m < M; m++) lay_chk[fill[layer_of[m]]++] = m;
		lay_nbr.assign((size_t)E * NBL_LAYER_ROW, 0);
		for (int ce = 0; ce < E; ce++) {
			const int n = c_var[ce], e0 = voff[n], dv = voff[n + 1] - e0;
			lay_nbr[(size_t)ce * NBL_LAYER_ROW] = n;
			lay_nbr[(size_t)ce * NBL_LAYER_ROW + 1] = dv;
			for (int k = 0; k < dv; k++) lay_nbr[(size_t)ce * NBL_LAYER_ROW + 4 + k] = v_cpos[e0 + k];
		}
	}

	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail_create(nullptr, NBL_ERR_NO_DEVICE, "no HIP device (this library has no CPU decode path)");
	if (device < 0 || device >= ndev) return fail_create(nullptr, NBL_ERR_ARG, "device index out of range");

	nbl_decoder *d = new nbl_decoder();
	d->device = device;
	d->prm = *params;
	if (params->method == NBL_METHOD_BS_TEMS) d->ext = *ext;
	if (hipSetDevice(device) != hipSuccess) return fail_create(d, NBL_ERR_HIP, "hipSetDevice failed");
	if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) return fail_create(d, NBL_ERR_HIP, "hipStreamCreate failed");
	if (const char *e = getenv("NBL_GRAPH")) d->use_graph = atoi(e) != 0;
	if (const char *e = getenv("NBL_COMPACT")) d->use_compact = atoi(e) != 0;
	if (const char *e = getenv("NBL_DEFER_LAST")) d->defer_last = atoi(e) != 0;
	d->g.N = N; d->g.M = M; d->g.E = E; d->g.q = q; d->g.p = p; d->g.poly = poly; d->g.maxdc = maxdc; d->g.maxdv = maxdv;
	std::vector<uint8_t> mul8((size_t)q * q);
	for (size_t i = 0; i < mul8.size(); i++) mul8[i] = (uint8_t)gf_mul[i];
	nbl_status st;
	if ((st = upload(d, voff, &d->g.voff)) || (st = upload(d, coff, &d->g.coff)) || (st = upload(d, v_cpos, &d->g.v_cpos)) ||
	    (st = upload(d, c_epos, &d->g.c_epos)) || (st = upload(d, c_var, &d->g.c_var)) || (st = upload(d, c_h, &d->g.c_h)) ||
	    (st = upload(d, c_hinv, &d->g.c_hinv)) || (st = upload(d, mul8, &d->g.mul)))
		return fail_create(d, st, "");
	if (osd_on) {
		if ((st = upload(d, osd_words, &d->osd.H))) return fail_create(d, st, "");
		d->osd_on = true;
		d->osd.R = osd_R;
		d->osd.n_dist = (int)(N * std::log((double)q) / std::log(2.0)); // compute_min_distance_bit's CodeLen_bit, truncated like it
		d->osd.order = osd->order < 0 ? 0 : osd->order; // (method 6 runs order 0 when the profile's order is -1)
		d->osd.flag = params->method == NBL_METHOD_OSD ? 1 : osd->flag;
		d->osd_factor = osd->factor;
		d->osd_acc = d->osd.flag == 0;
	}
	if (lay) {
		if ((st = upload(d, lay_chk, &d->ly.chk)) || (st = upload(d, lay_nbr, &d->ly.nbr))) return fail_create(d, st, "");
		d->layered = true;
		d->n_layers = n_layers;
		d->h_layer_of = layer_of;
		d->h_lay_off = lay_off;
	}
	d->kind = kind;
	d->h_coff = coff; d->h_cvar = c_var; d->h_ch = c_h;
	d->h_mul.assign(gf_mul, gf_mul + (size_t)q * q);
	d->d_e2c_map = (int *)d->g.v_cpos;
	d->shape = shape;
	if (shape.has_ems_toff()) {
		// permutation offsets of the specialised EMS kernel: variable-domain symbol a of lane l -> byte offset of h*a in a q-vector
		std::vector<unsigned long long> toff((size_t)E * 64);
		for (int ce = 0; ce < E; ce++)
			for (int l = 0; l < 64; l++) {
				unsigned long long pk = 0;
				for (int i = 0; i < 4; i++) {
					const int a = 2 * l + (i & 1) + 128 * (i >> 1);
					pk |= (unsigned long long)(8u * gf_mul[(size_t)c_h[ce] * q + a]) << (16 * i);
				}
				toff[(size_t)ce * 64 + l] = pk;
			}
		if ((st = upload(d, toff, &d->g.ems_toff))) return fail_create(d, st, "");
	}
	if (shape.has_dv2_row()) {
		std::vector<int> row((size_t)M * 16);
		for (int m = 0; m < M; m++)
			for (int j = 0; j < 4; j++) {
				const int ce = coff[m] + j, n = c_var[ce], e = c_epos[ce], e0 = voff[n];
				row[(size_t)m * 16 + j] = n;
				row[(size_t)m * 16 + 4 + j] = v_cpos[e0];
				row[(size_t)m * 16 + 8 + j] = v_cpos[e0 + 1];
				row[(size_t)m * 16 + 12 + j] = e | ((e == e0) ? (int)0x80000000 : 0);
			}
		if ((st = upload(d, row, &d->g.dv2_row))) return fail_create(d, st, "");
	}
	if (shape.has_c_nbr()) {
		// fused small-field iteration: everything the variable-node stage of a check-major edge needs, in one 16-byte row
		// (variable degrees 2 and 3 only: the fused loaders add the second c2v vector unconditionally; a code with a degree-1
		// variable takes the separate variable-node launch, which handles any degree)
		std::vector<int> nbr((size_t)E * 4);
		for (int ce = 0; ce < E; ce++) {
			const int n = c_var[ce], e0 = voff[n], dv = voff[n + 1] - e0;
			for (int k = 0; k < 3; k++) nbr[(size_t)ce * 4 + k] = k < dv ? v_cpos[e0 + k] : -1;
			nbr[(size_t)ce * 4 + 3] = (c_epos[ce] == e0) ? 1 : 0;
		}
		if ((st = upload(d, nbr, &d->g.c_nbr))) return fail_create(d, st, "");
	}
	void *cnt = nullptr;
	if (hipMalloc(&cnt, 16) != hipSuccess) return fail_create(d, NBL_ERR_NOMEM, "hipMalloc failed");
	d->graph_allocs.push_back(cnt);
	d->w.n_done = (int *)cnt;
	d->w.n_act = (int *)cnt + 1;
	if (hipEventCreate(&d->ev[0]) != hipSuccess || hipEventCreate(&d->ev[1]) != hipSuccess) return fail_create(d, NBL_ERR_HIP, "hipEventCreate failed");
	if (params->max_batch > 0 && (st = ensure_workspace(d, params->max_batch))) return fail_create(d, st, "");
	*out = d;
	return NBL_OK;
}
