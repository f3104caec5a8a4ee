// AP matching pieces shared by the box form (score.hip, hdy_ap_match) and the mask form (mask_score.hip, hdy_mask_ap_match): the two differ in
// where a pair's IoU comes from and agree, word for word, in rules 3-5 (include/hdyolo.h "detection scoring"), so those exist once.
#pragma once
#include "common.h"

// is `label` one of the n_ign ignored labels
__device__ __forceinline__ bool ap_ignored(const long long* ign, int n_ign, long long label) {
    bool ig = false;
    for (int k = 0; k < n_ign; ++k) ig |= ign[k] == label;
    return ig;
}

// rule 3's claim on a truth: the 64-bit atomic MINIMUM of these keys is the prediction of highest score, on a tie the lower row
__device__ __forceinline__ unsigned long long ap_claim_key(float score, unsigned row) {
    return ((unsigned long long)desc_key(score) << 32) | row;
}

// rules 4 and 5 for prediction p, whose match[p] / match_iou[p] / live[p] hold rule 2's result (best truth or -1, its IoU, touched) and are
// rewritten as the outputs; `row` is p's row in the tie rule, `claim` the claims of rule 3
__device__ __forceinline__ void ap_resolve(int p, unsigned row, const float* __restrict__ ps, const long long* __restrict__ pl,
                                           const long long* __restrict__ tl, const unsigned long long* __restrict__ claim, const float* iouv,
                                           int n_iou, unsigned short* hit, unsigned char* live, int* match, float* miou) {
    const int best = match[p];
    const float iou = miou[p];
    const bool touched = live[p] != 0;
    bool matched = false;
    if (best >= 0) matched = claim[best] == ap_claim_key(ps[p], row) && pl[p] == tl[best];
    unsigned bits = 0;
    if (matched)
        for (int j = 0; j < n_iou; ++j) bits |= (iou >= iouv[j] ? 1u : 0u) << j;
    hit[p] = (unsigned short)bits;
    live[p] = (touched && !matched) ? 0 : 1;
    match[p] = matched ? best : -1;
    miou[p] = matched ? iou : 0.f;
}
