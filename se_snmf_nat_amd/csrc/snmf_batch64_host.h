// snmf_batch64_host.h -- what snmf_tu_batch.hip (the snmf_batch handle and the C entries) and snmf_tu_batch64.hip (the fp64
// state of such a handle) share on the host.  A handle made by snmf_batch_create_fp64 carries a Batch64 and every
// snmf_batch_* entry hands over to the function of the same name here; an fp32 handle carries none.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct snmf_ctx;
struct snmf_params;
struct Batch64;

// Validates like snmf_batch_create (the refusals come before the device is touched), checks the grid and memory limits
// before anything is allocated, then allocates and builds the tables.
int batch64_create(snmf_ctx* ctx, const snmf_params* p, int32_t n_problems, const int32_t* T, Batch64** out);
void batch64_destroy(Batch64* b);
int batch64_set_sparsity(Batch64* b, const double* sparsity);
int batch64_set_problem(Batch64* b, int32_t k, const double* V, int64_t ldV, const double* W0, const double* H0);
int batch64_set_problem(Batch64* b, int32_t k, const float* V, int64_t ldV, const float* W0, const float* H0);
int batch64_run(Batch64* b, int32_t n_iters);
int batch64_get(Batch64* b, int32_t k, double* W, double* H, double* div_out, double* cost_out, int32_t* n_iter_out);
int batch64_get(Batch64* b, int32_t k, float* W, float* H, double* div_out, double* cost_out, int32_t* n_iter_out);
int batch64_describe(const Batch64* b, char* buf, size_t buflen);
