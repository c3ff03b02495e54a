// snmf_online_classes.h -- host-side helpers of the online separators: the FFT-size dispatch of their transform kernels, and
// the class partition (snmf_online_set_classes / snmf_online_batch_set_classes, include/snmf.h): p.EVENT_NUM / p.EVENT_RANK / p.NOISE_NUM / p.NOISE_RANK of
// settings/initial_setting_SNMF_NAT.m:40-44 -> the column ranges the class kernels walk (snmf_online_common.h: oclass_dft).
// Shared by snmf_tu_online.hip, snmf_tu_online_f64.hip and snmf_tu_online_batch.hip.
#pragma once
#include "snmf_internal.h"

// the transform kernels are templates on LOGN = log2(fftlength), 6 .. 12 (checked at creation): f(integral_constant<int, LOGN>)
template <typename K>
static inline void by_logn(K&& f, int N) {
    switch (N) {
        case 64: f(std::integral_constant<int, 6>{}); break;
        case 128: f(std::integral_constant<int, 7>{}); break;
        case 256: f(std::integral_constant<int, 8>{}); break;
        case 512: f(std::integral_constant<int, 9>{}); break;
        case 1024: f(std::integral_constant<int, 10>{}); break;
        case 2048: f(std::integral_constant<int, 11>{}); break;
        default: f(std::integral_constant<int, 12>{}); break;
    }
}

// Ranks are 1-based starts (src/bnmf_sep_event_RT_IS16.m:158-163, :180-185): event class i covers columns
// EVENT_RANK(i) .. EVENT_RANK(i+1)-1 of B_x, the last one up to R_x; noise class i the same of B_d.  On success cls holds
// event_num + noise_num + 1 ascending 0-based column indices over [B_x | B_d], cls.back() = R_x + R_d.
//   SNMF_ERR_INVALID      a count below 1, a NULL list, a rank below 1, ranks not strictly ascending, a start beyond R_x / R_d
//   SNMF_ERR_UNSUPPORTED  a first rank above 1 (Xm_hat_sum = the sum over the classes feeds the gain, :201: the reference would
//                         silently drop the leading columns from the filter), more than kOClassMax classes on a side
static inline int online_class_ranges(int32_t event_num, const int32_t* event_rank, int32_t noise_num, const int32_t* noise_rank,
                                      int R_x, int R_d, std::vector<int>* cls) {
    if (event_num < 1 || noise_num < 1 || !event_rank || !noise_rank) return fail(SNMF_ERR_INVALID, "class partition: need EVENT_NUM, NOISE_NUM >= 1 and both rank lists");
    const struct { const char* nm; int32_t n; const int32_t* rk; int R; } side[2] = {{"EVENT_RANK", event_num, event_rank, R_x},
                                                                                   {"NOISE_RANK", noise_num, noise_rank, R_d}};
    for (const auto& s : side)
        for (int i = 0; i < s.n; ++i) {
            if (s.rk[i] < 1 || s.rk[i] > s.R) return fail(SNMF_ERR_INVALID, "%s(%d) = %d outside [1, %d]", s.nm, i + 1, s.rk[i], s.R);
            if (i > 0 && s.rk[i] <= s.rk[i - 1]) return fail(SNMF_ERR_INVALID, "%s must be strictly ascending", s.nm);
        }
    for (const auto& s : side) {
        if (s.rk[0] != 1) return fail(SNMF_ERR_UNSUPPORTED, "%s(1) = %d: the classes must cover the dictionary from column 1 (their sum feeds the gain)", s.nm, s.rk[0]);
        if (s.n > kOClassMax) return fail(SNMF_ERR_UNSUPPORTED, "%d classes on a side, at most %d", s.n, kOClassMax);
    }
    cls->clear();
    for (int i = 0; i < event_num; ++i) cls->push_back(event_rank[i] - 1);
    for (int i = 0; i < noise_num; ++i) cls->push_back(R_x + noise_rank[i] - 1);
    cls->push_back(R_x + R_d);
    return SNMF_OK;
}
