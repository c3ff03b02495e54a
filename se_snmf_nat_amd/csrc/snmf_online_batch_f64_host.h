// snmf_online_batch_f64_host.h -- host interface between snmf_tu_online_batch.hip (owner of the snmf_online_batch handle) and
// snmf_tu_online_batch_f64.hip (the fp64 batch behind it, kernels in snmf_online_batch_f64.h).  Declarations only.
#pragma once
#include "snmf.h"

struct OnlineBatchF64;
// `p`, S and every entry of `settings` have passed snmf_tu_online_batch.hip's validation; the arrays are
// snmf_online_batch_create's, in fp64.  Bx: F x Rx, or with bx_per_stream F x Rx x S; settings: [S] or NULL = p for all
int online_batch_f64_create(snmf_ctx* ctx, const snmf_online_params* p, int32_t S, const double* Bx, int bx_per_stream, const double* Bd0,
                            const double* H0, const double* Ad0, const snmf_online_stream_settings* settings, const double* win_stft,
                            const double* win_istft, OnlineBatchF64** out);
void online_batch_f64_destroy(OnlineBatchF64* o);
// xhi / dhi: the class signals (snmf_online_batch_process_classes_f64), class-major at cap[s], or NULL
int online_batch_f64_process(OnlineBatchF64* o, const double* const* pcm, const int64_t* n, const int32_t* flush, double* const* xt,
                             int16_t* const* xt_i16, double* const* xh, double* const* dh, double* const* xhi, double* const* dhi,
                             const int64_t* cap, int64_t* n_out);
int online_batch_f64_set_classes(OnlineBatchF64* o, int32_t event_num, const int32_t* event_rank, int32_t noise_num,
                                 const int32_t* noise_rank);
// Bx n x Rx x F or NULL (keep), Bd n x Rd x F or NULL (carry), H0 n x r or NULL, Ad n x Ra x ma or NULL, settings [n]
// (validated) or NULL (keep)
int online_batch_f64_restart(OnlineBatchF64* o, int32_t n, const int32_t* slots, const double* Bx, const double* Bd, const double* H0,
                             const double* Ad, const snmf_online_stream_settings* settings);
int online_batch_f64_get_settings(OnlineBatchF64* o, int32_t k, snmf_online_stream_settings* out);
void online_batch_f64_dims(OnlineBatchF64* o, int* r, int* ra_ma);  // lengths of one stream's H0 and Ad_blk0
int online_batch_f64_idle(const OnlineBatchF64* o);  // obatch_idle_check: SNMF_ERR_STATE on a failed batch or a stream mid-recording
int online_batch_f64_get_basis(OnlineBatchF64* o, int32_t k, double* Bd, int64_t ld);
int online_batch_f64_trace(OnlineBatchF64* o, int32_t k, snmf_online_frame* out, int64_t cap, int64_t* n);
// get-state / set-state (snmf_online_batch_state_info / _get_state / _set_state) of the fp64 batch
void online_batch_f64_state_info(OnlineBatchF64* o, snmf_online_state_info* out);
int online_batch_f64_get_state(OnlineBatchF64* o, int32_t n, const int32_t* slots, void* records, int64_t cap);
int online_batch_f64_set_state(OnlineBatchF64* o, int32_t n, const int32_t* slots, const void* records, int64_t bytes);
