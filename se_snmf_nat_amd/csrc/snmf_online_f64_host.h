// snmf_online_f64_host.h -- host interface between snmf_tu_online.hip (owner of the snmf_online handle) and
// snmf_tu_online_f64.hip (the fp64 separator behind it, kernels in snmf_online_f64.h).  Declarations only.
#pragma once
#include "snmf.h"

struct OnlineF64;
int online_f64_create(snmf_ctx* ctx, const snmf_online_params* p, const double* Bx, const double* Bd, const double* H0,
                      const double* Ad0, const double* win_stft, const double* win_istft, OnlineF64** out);
void online_f64_destroy(OnlineF64* o);
// xhi / dhi: the class signals (snmf_online_process_classes_f64), class-major at `cap`, or NULL
int online_f64_process(OnlineF64* o, const double* pcm, int64_t n, int flush, double* xt, int16_t* xt_i16, double* xh, double* dh,
                       double* xhi, double* dhi, int64_t cap, int64_t* n_out);
int online_f64_set_classes(OnlineF64* o, int32_t event_num, const int32_t* event_rank, int32_t noise_num, const int32_t* noise_rank);
void online_f64_class_counts(OnlineF64* o, int* n_event, int* n_noise);  // (1, 1) without a partition
int online_f64_get_basis(OnlineF64* o, double* Bd, int64_t ld);
int online_f64_trace(OnlineF64* o, snmf_online_frame* out, int64_t cap, int64_t* n);
// the state g as a record, and the next file in place (snmf_online_stream_state_info / _get_state / _set_state / _restart_f64)
void online_f64_state_info(OnlineF64* o, snmf_online_state_info* out);
int online_f64_get_state(OnlineF64* o, void* record, int64_t cap);
int online_f64_set_state(OnlineF64* o, const void* record, int64_t bytes);
int online_f64_restart(OnlineF64* o, const double* Bd, const double* H0, const double* Ad);
