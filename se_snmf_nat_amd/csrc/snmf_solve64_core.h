// snmf_solve64_core.h -- the device-resident core of the fp64 solve (defined in snmf_tu_solve64.hip), for the callers that
// keep their matrices in HBM between solves (snmf_tu_train64.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "snmf.h"

// bytes of device workspace one solve of `p` needs; validates p and its update masks (src/sparse_nmf.m:142-148, :176-179)
int solve64_ws_bytes(const snmf_params* p, size_t* bytes);
// src/sparse_nmf.m:157-286 on device pointers, all tight column-major: dV F x T (floored in place when p->floor_v), dW F x r
// and dH r x T in / out, dS the sparsity array of p->sparsity_kind (NULL for a scalar); the update masks come with p.
// ws: at least solve64_ws_bytes(p) bytes, the caller's -- solves that run one after the other may share one block sized
// for the largest.  The objective vectors (max_iter entries each, may be NULL) and n_iter go to the host; the context's
// stream is idle on return.
int solve64_core(snmf_ctx* ctx, const snmf_params* p, double* dV, double* dW, double* dH, const double* dS, void* ws, size_t ws_bytes,
                 double* div_out, double* cost_out, int32_t* n_iter_out);
// The missing-data solve (src/snmf_mdi.m:163-306, src/snmf_mdi_Sm.m likewise): solve64_core with a resident mask dM (F x T, tight
// column-major, 1 = observed, soft masks in [0, 1]).  dV starts as max(dV .* dM, flr) (:175; p->floor_v is not read), is
// re-imputed after the W step of every iteration (:251-254) -- so it holds the imputed v on return -- and the gain-matched
// v_MDI (:296-306) goes to dVm (F x T tight; it may be dV itself).  p->conv_eps and the sparsity carry conv_eps_mdi and
// sparsity_mdi.  The workspace is that of solve64_core: solve64_ws_bytes(p).  Neither factor updated is a solve as well:
// lambda stays the initial w * h, the imputation and the gain step run.
int solve64_mdi_core(snmf_ctx* ctx, const snmf_params* p, double* dV, const double* dM, double* dW, double* dH, const double* dS, void* ws,
                     size_t ws_bytes, double* dVm, double* div_out, double* cost_out, int32_t* n_iter_out);
