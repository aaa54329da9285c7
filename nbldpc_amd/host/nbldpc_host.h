// nbldpc_amd/host/nbldpc_host.h -- CNBLDPC with the reference's public interface (NBLDPC.h:13-71) on top of the C ABI.
//
//   bool Initial(CSimulation&)                          NBLDPC.h:42   code-file parse, puncture list, encoder, nbl_create
//   int  Encode(int* msg_sym, int* code_sym)            NBLDPC.h:61   systematic encode (also rewrites msg_sym, :598-601)
//   int  Decoding(double** L_ch, int* out, int*, int*)  NBLDPC.h:71   one codeword (batch of one)
//   int  DecodingBatch(...)                             new            B codewords, ONE device call
// All decoding happens in libnbldpc_hip.so; this class holds no CPU decoder.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/nbldpc.h"
#include "gf.h"
#include "simulation.h"

class CNBLDPC {
public:
	CNBLDPC() = default;
	~CNBLDPC();
	CNBLDPC(const CNBLDPC &) = delete;
	CNBLDPC &operator=(const CNBLDPC &) = delete;

	int GFq = 0;
	CGF GF;
	int maxIter = 0;
	int CodeLen = 0, ChkLen = 0, PunctureLen = 0;
	std::vector<int> PuncturePositionV;
	int *PuncturePosition = nullptr; // = PuncturePositionV.data()
	int maxVarDegree = 0, maxChkDegree = 0;
	std::vector<int> VarDegree, ChkDegree;
	std::vector<std::vector<int>> VarLink, ChkLink, VarLinkGFe, ChkLinkGFe;
	int DecodeMethod = 0;

	bool Initial(CSimulation &sim, int device = 0, int fixed_iters = 0); // device < 0: graph + encoder only, no GPU touched
	int Encode(int *msg_sym, int *code_sym);
	int Decoding(double **L_ch, int *DecodeOutput, int *RelySeri_symbol, int *RelySeri_bit);
	// L_ch [B][CodeLen][GFq-1]; out [B][CodeLen]; converged [B] (may be null); iters [B] (may be null). 0 on success.
	int DecodingBatch(const double *L_ch, int B, int *out, uint8_t *converged, int *iters);
	// device-side demodulation (replaces CComm::Demodulate, Comm.cpp:340-407): rx [B][L][2] received samples
	int SetDemodulator(int mod_order, int n_mod_sym, const double *constellation, const int *src, int metric = 0); // metric: NBL_DEMOD_*, general orders only
	// gain [B][L][2] (may be null): coherent reception over a flat-fading channel (nbl_decode_batch_samples_csi / _idd_csi)
	int DecodingBatchSamples(const double *rx, double sigma, int B, int *out, uint8_t *converged, int *iters, const double *gain = nullptr);
	// the device-side channel's fading model (nbl_set_fading): model NBL_FADING_*, coherence in samples
	int SetFading(int model, int coherence);
	uint64_t ChannelDraws() const { return dec ? nbl_channel_draws(dec) : 0; } // uniform draws a frame moves a lane's generator
	// per-bit LLRs in place of symbol LLRs (the RX_LLR_BIT -> RX_LLR_SYM loop of Comm.cpp:359-373 runs on the device): bit_llr [B][CodeLen p],
	// ln P(bit = 1) / P(bit = 0), bit j of a symbol has value 2^j, a punctured bit is 0.0.  No demodulator has to be set.
	int DecodingBatchBits(const double *bit_llr, int B, int *out, uint8_t *converged, int *iters);
	// a-posteriori LLRs of the last Decoding* call, all B codewords: sym_llr [B][CodeLen][GFq-1] and / or bit_llr [B][CodeLen p] (either
	// may be null, not both); metric: NBL_SOFT_* (0 log-sum, 1 max-log).  Defined in include/nbldpc.h.
	int SoftOutput(int metric, double *sym_llr, double *bit_llr);
	// device-side channel (replaces CComm::Channel_AWGN + CRand, Comm.cpp:328-337 / Rand.cpp:17-37): tx_index [B][L] constellation
	// indices, lane_state [B][3] generator states in front of the frame
	int DecodingBatchNoise(const unsigned char *tx_index, const unsigned int *lane_state, double sigma, int B, int *out, uint8_t *converged, int *iters);
	// the same in two phases (slot 0 / 1): the channel of cycle k+1 may run while cycle k is decoded
	int ChannelBatch(int slot, const unsigned char *tx_index, const unsigned int *lane_state, double sigma, int B);
	int DecodingBatchResident(int slot, double sigma, int B, int *out, uint8_t *converged, int *iters);
	// the encoder as a dense linear map, gen [CodeLen][K]: code[n] = sum_k gen[n][k] * msg[k] (K unit encodes; Encode is GF(q)-linear),
	// the final column exchanges included.  Builds the encoder first if the profile did not ask for one (Random Msg: 0).
	bool Generator(std::vector<uint16_t> &gen);
	// device-side transmit chain and error count (include/nbldpc.h: nbl_set_transmitter / nbl_transmit_batch / nbl_count_errors)
	int SetTransmitter(const uint16_t *gen, int crc_len, int random_msg, int parallel, int mod_order, int n_mod_sym);
	int TransmitBatch(int slot, const uint16_t *pn_state, const unsigned int *lane_state, double sigma, int B);
	int CountErrors(int slot, int B, int *err_sym, int *err_bit, uint8_t *crc_ok);
	const std::string &LastError() const { return error; }
	nbl_decoder *Handle() const { return dec; }
	int IddPasses() const { return idd_passes; } // NBL_IDD_PASSES as Initial read it

private:
	// encoder state (InitialEncode NBLDPC.cpp:477-560)
	std::vector<int> swap_src, swap_dst;
	std::vector<std::vector<int>> enc_link, enc_coef;
	bool InitialEncode();
	bool LoadMatRepr(std::vector<uint8_t> &m);
	nbl_decoder *dec = nullptr;
	std::string error;
	// NBL_IDD_PASSES=k (default 1), NBL_IDD_SOFT=maxlog|logsum: DecodingBatchSamples and DecodingBatchResident go through the
	// iterative-demapping loop (nbl_decode_batch_samples_idd / nbl_decode_batch_resident_idd); above 1 needs a general demodulator
	int idd_passes = 1, idd_soft = NBL_SOFT_MAXLOG;
};
