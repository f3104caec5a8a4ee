// AP matching shared by the box form (score.hip, hdy_ap_match) and the mask form (mask_score.hip, hdy_mask_ap_match): the two differ in where a
// pair's IoU comes from and agree, word for word, in rules 3-5 (include/hdyolo.h "detection scoring"), so the rule block, its argument checks
// and those rules exist once.
#pragma once
#include "common.h"

constexpr int AP_MAX_IOU = 16, AP_MAX_IGNORE = 4;      // thresholds (the bits of hit) and ignored labels of one call

// What rules 3-5 read and write, the same in both forms: scores and labels of the concatenated rows, the optional rows of the tie rules, the
// thresholds (padded with 2.0, which no IoU reaches) and ignored labels by value, the four outputs and rule 3's claim word per truth.  The
// kernel argument blocks of both forms start with it (Args, MArgs) and add where their IoU comes from.
struct ApRules {
    const float* ps; const long long *pl, *tl; const int *prow, *trow;
    int n_iou, n_ign;
    float pair_iou;
    float iouv[AP_MAX_IOU];
    long long ign[AP_MAX_IGNORE];
    unsigned short* hit; unsigned char* live; int* match; float* miou;
    unsigned long long* claim;

    // the row of prediction p / truth t in the tie rules
    __device__ __forceinline__ int pred_row(int p) const { return prow ? prow[p] : p; }
    __device__ __forceinline__ int true_row(int t) const { return trow ? trow[t] : t; }
};

// is `label` one of the ignored labels
__device__ __forceinline__ bool ap_ignored(const ApRules& r, long long label) {
    bool ig = false;
    for (int k = 0; k < r.n_ign; ++k) ig |= r.ign[k] == label;
    return ig;
}

// rule 3's claim on a truth: the 64-bit atomic MINIMUM of these keys is the prediction of highest score, on a tie the lower row
__device__ __forceinline__ unsigned long long ap_claim_key(float score, unsigned row) {
    return ((unsigned long long)desc_key(score) << 32) | row;
}

// rules 4 and 5 for prediction p, whose match[p] / miou[p] / live[p] hold rule 2's result (best truth or -1, its IoU, touched) and are
// rewritten as the outputs
__device__ __forceinline__ void ap_resolve(const ApRules& r, int p) {
    const int best = r.match[p];
    const float iou = r.miou[p];
    const bool touched = r.live[p] != 0;
    bool matched = false;
    if (best >= 0) matched = r.claim[best] == ap_claim_key(r.ps[p], (unsigned)r.pred_row(p)) && r.pl[p] == r.tl[best];
    unsigned bits = 0;
    if (matched)
        for (int j = 0; j < r.n_iou; ++j) bits |= (iou >= r.iouv[j] ? 1u : 0u) << j;
    r.hit[p] = (unsigned short)bits;
    r.live[p] = (touched && !matched) ? 0 : 1;
    r.match[p] = matched ? best : -1;
    r.miou[p] = matched ? iou : 0.f;
}

// The argument checks of the rule block (n_pred / n_true rows, already known to be non-negative); the entry points add those of their own
// arguments.  Host code: iouv and ignore are host arrays, everything else a device pointer that is only looked at.
inline int ap_check_rules(const char* who, int n_pred, int n_true, const float* pred_scores, const long long* pred_labels, const int* pred_row,
                          const long long* true_labels, const int* true_row, const float* iouv, int n_iou, float pair_iou, const long long* ignore,
                          int n_ignore, const unsigned short* hit, const unsigned char* live, const int* match, const float* match_iou) {
    HDY_ARG(n_iou >= 1 && n_iou <= AP_MAX_IOU, "%s: n_iou=%d outside [1, %d]", who, n_iou, AP_MAX_IOU);
    HDY_ARG(n_ignore >= 0 && n_ignore <= AP_MAX_IGNORE, "%s: n_ignore=%d outside [0, %d]", who, n_ignore, AP_MAX_IGNORE);
    HDY_ARG(iouv && (ignore || n_ignore == 0), "%s: null threshold or ignore array (host pointers)", who);
    HDY_ARG(pair_iou > 0.f && pair_iou <= 1.f, "%s: pair_iou must be in (0, 1]", who);
    HDY_ARG(n_pred == 0 || (pred_scores && pred_labels && hit && live && match && match_iou), "%s: null prediction or output pointer", who);
    HDY_ARG(n_true == 0 || true_labels, "%s: null truth pointer", who);
    HDY_ARG((((uintptr_t)pred_labels | (uintptr_t)true_labels) & 7) == 0, "%s: labels must be 8-byte aligned", who);
    HDY_ARG((((uintptr_t)pred_scores | (uintptr_t)pred_row | (uintptr_t)true_row | (uintptr_t)match | (uintptr_t)match_iou) & 3) == 0 &&
            ((uintptr_t)hit & 1) == 0, "%s: misaligned pointer", who);
    return HDY_OK;
}

// the rule block from checked arguments (the claim words lie in the entry point's workspace)
inline void ap_fill_rules(ApRules& r, const float* pred_scores, const long long* pred_labels, const int* pred_row, const long long* true_labels,
                          const int* true_row, const float* iouv, int n_iou, float pair_iou, const long long* ignore, int n_ignore,
                          unsigned short* hit, unsigned char* live, int* match, float* match_iou, unsigned long long* claim) {
    r.ps = pred_scores; r.pl = pred_labels; r.tl = true_labels; r.prow = pred_row; r.trow = true_row;
    r.n_iou = n_iou; r.n_ign = n_ignore; r.pair_iou = pair_iou;
    for (int j = 0; j < AP_MAX_IOU; ++j) r.iouv[j] = j < n_iou ? iouv[j] : 2.f;
    for (int j = 0; j < AP_MAX_IGNORE; ++j) r.ign[j] = j < n_ignore ? ignore[j] : 0;
    r.hit = hit; r.live = live; r.match = match; r.miou = match_iou; r.claim = claim;
}
