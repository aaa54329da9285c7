// nbldpc_amd/csrc/nbl_plan.h -- the one place where a shape meets a check-node kernel (nbl_plan.cpp; pure host code, no HIP)
#pragma once
#include "../../include/nbldpc.h"
#include "nbl_common.h"

enum NblCn {
	NBL_CN_EMS256, NBL_CN_EMS_SMALL, NBL_CN_EMS64, NBL_CN_EMS,
	NBL_CN_TEMS64, NBL_CN_TEMS256, NBL_CN_TEMS_SMALL, NBL_CN_TEMS,
	NBL_CN_BP256, NBL_CN_BP64, NBL_CN_BP_SMALL, NBL_CN_BP,
	NBL_CN_BSTEMS, NBL_CN_EMS_LAYERED, NBL_CN_TEMS_LAYERED,
	NBL_CN_NONE, // method 6: no iteration
	NBL_CN_BP_LAYERED,
	NBL_CN_FHT, NBL_CN_FHT_LAYERED, // nbl_create_fht: the FHT sum-product check node, flooding and layered
	NBL_CN_FHT_WIDE, NBL_CN_FHT_WIDE_LAYERED, // the same in the degree-independent layout: codes with a check above degree NBL_MAXDC
	NBL_CN_EMS_WIDE, NBL_CN_EMS_WIDE_LAYERED, // nbl_create_ems_wide: EMS, one check per workgroup, any check degree up to NBL_EMS_MAX_CHECK_DEGREE
	NBL_CN_TEMS_WIDE, NBL_CN_TEMS_WIDE_LAYERED, // nbl_create_tems_wide: T-EMS, one check per workgroup, 64-bit path code, check degrees up to NBL_TEMS_MAX_CHECK_DEGREE
	NBL_CN_BP_WIDE, NBL_CN_BP_WIDE_LAYERED, // nbl_create_bp_wide: exact log-QSPA, one check per workgroup, check degrees up to NBL_BP_MAX_CHECK_DEGREE
	NBL_CN_COUNT
};

struct NblPlan {
	NblCn cn;      // the check-node kernel of every iteration
	bool fusable;  // the shape has a fused iteration (variable-node pass inside cn): c2v_alt and c2v_zero exist
	bool fused;    // this decode runs it
	bool want_v2c; // v2c exists in HBM: something reads it (the unfused path, the damped methods, state read-back)
	bool f32;      // nbl_create_fht32 / nbl_create_fht32_wide: cn (fht, fht_layered, fht_wide or fht_wide_layered) is run by its binary32
	               // instance on the float message state; named fht32 / fht32_layered / fht32_wide / fht32_wide_layered
	bool minmax;   // nbl_create_minmax: cn (ems_wide or ems_wide_layered: the launch shape, the input formers of nbl_cn_shell.h and the buffers are those) is run
	               // by the Min-Max programme (nbl_cn_minmax.hip); named minmax / minmax_layered.  A flag beside cn, as f32 is: NblCn lists
	               // the kernels tests/test_idd_kinds.py wants a loop cell for, and Min-Max pins its loop in tests/test_gpu_minmax.py
};

// Which entry point made the decoder.  The kinds exclude one another; each non-base kind runs one method (nbl_entries, nbl_decoder.h):
//   BASE       nbl_create* / nbl_create_layered*: the precedence of nbl_plan.cpp; force_generic 1 = the general kernel, 2 = the
//              specialised one, neither fused; 3 changes nothing
//   FHT        nbl_create_fht (method 1): fht / fht_layered; a code with a check above degree NBL_MAXDC runs fht_wide / fht_wide_layered,
//              and force_generic 3 selects that wide programme at any check degree (so that the two layouts can be compared on the same
//              inputs); 0, 1, 2 change nothing
//   FHT32      nbl_create_fht32 (method 1): the check-node kinds fht / fht_layered in binary32 (NblPlan::f32), never fused, with v2c (the
//              float one); no debug switch moves it
//   EMS_WIDE   nbl_create_ems_wide (method 2): a code with a check above degree NBL_MAXDC runs ems_wide / ems_wide_layered under every
//              switch; any other code gets the plan of nbl_create / nbl_create_layered, except that force_generic 3 selects the wide
//              programme
//   TEMS_WIDE  nbl_create_tems_wide (method 4): a code with a check above degree NBL_MAXDC or with log2(q) maxdc > 32 (the path does not
//              fit tems_check_node's 32-bit code) runs tems_wide / tems_wide_layered under every switch; any other code gets the plan of
//              nbl_create / nbl_create_layered_ex, except that force_generic 3 selects the wide programme where
//              tems_nc <= NBL_TEMS_WIDE_MAX_NC
//   BP_WIDE    nbl_create_bp_wide (method 1): a code with a check above degree NBL_MAXDC runs bp_wide / bp_wide_layered under every
//              switch; any other code gets the plan of nbl_create / nbl_create_layered_bp, except that force_generic 3 selects the wide
//              programme
//   FHT32_WIDE nbl_create_fht32_wide (method 1): a code with a check above degree NBL_MAXDC runs fht_wide / fht_wide_layered in binary32
//              (NblPlan::f32; named fht32_wide / fht32_wide_layered) under every switch; any other code gets the plan of
//              nbl_create_fht32, except that force_generic 3 selects the wide programme
//   MINMAX     nbl_create_minmax (method 3): minmax / minmax_layered (NblPlan::minmax), one programme for every check degree and field;
//              never fused; flooding keeps v2c, layered has none; no debug switch moves it
enum NblKind { NBL_KIND_BASE, NBL_KIND_FHT, NBL_KIND_FHT32, NBL_KIND_EMS_WIDE, NBL_KIND_TEMS_WIDE, NBL_KIND_BP_WIDE, NBL_KIND_FHT32_WIDE, NBL_KIND_MINMAX };
// the kinds whose iterations run on the float message state (NblWork32): the float workspace, widen_state, the binary32 launchers
inline bool nbl_kind_f32(NblKind kind) { return kind == NBL_KIND_FHT32 || kind == NBL_KIND_FHT32_WIDE; }

struct NblPlanReq {
	NblKind kind;
	bool layered;      // which of the kind's two schedules
	int force_generic; // nbl_debug_force_generic's value
	bool record_state; // nbl_set_record_state's
	bool small_on;     // the kernels NBL_NO_SMALL switches off (EMS-small, T-EMS-small, BP-small, EMS-64) may be chosen
};

NblShape nbl_shape(const nbl_code_desc *code);
NblPlan nbl_plan(const NblShape &s, const nbl_params &prm, const NblPlanReq &rq);
// the codes only the wide T-EMS programme runs (creation refuses tems_nc > NBL_TEMS_WIDE_MAX_NC there)
inline bool nbl_tems_needs_wide(const NblShape &s) { return s.maxdc > NBL_MAXDC || s.p * s.maxdc > 32; }
const char *nbl_cn_name(NblCn cn);
const char *nbl_plan_name(const NblPlan &plan); // nbl_cn_name(plan.cn), or fht32[_wide][_layered] for a binary32 plan, minmax[_layered] for a Min-Max plan

// What each specialised kernel can run, beside the kernel (its LDS arithmetic lives there); nbl_plan is the only caller.
// method: NBL_METHOD_* of include/nbldpc.h.  Unfused: any variable degrees.  Fused: NblShape::has_c_nbr for the small-field and the
// EMS-64 kernel, NblShape::has_dv2_row for the others.
bool nbl_ems256_applicable(const NblShape &s, int nm, int nc);             // nbl_cn_ems256.hip
bool nbl_small_applicable(const NblShape &s, int method, int nm, int nc);  // nbl_cn_small.hip: q <= 32, log-QSPA also q = 64
bool nbl_ems64_applicable(const NblShape &s, int nm, int nc);              // nbl_cn_ems64.hip
bool nbl_tems64_applicable(const NblShape &s, int nr, int nc);             // nbl_cn_tems64.hip
bool nbl_tems256_applicable(const NblShape &s, int nr, int nc);            // nbl_cn_tems256.hip
bool nbl_bp256_applicable(const NblShape &s);                              // nbl_cn_bp256.hip
bool nbl_bp64_applicable(const NblShape &s);                               // nbl_cn_bp64.hip
