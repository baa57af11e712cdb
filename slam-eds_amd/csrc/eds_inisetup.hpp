// The rest of CoarseInitializer::setFirst (include/eds_hip_inisetup.h): gridMaxSelection and makePixelStatus of the reference's
// src/init/CoarseInitializer.h (lines quoted as H:n), restated over the Px pyramid.  What the device kernels (eds_inisetup.hip) and the
// host share is the per-pixel rule (gms_scores), the cells' geometry, the order two candidates of one cell are ranked in (gms_better)
// and makePixelStatus's controller, which is host code on both sides and takes the pass as a callable.  grid_max_selection and
// make_pixel_status walk the reference's loops in the reference's order on the host; the device equals them bit for bit.  Every
// translation unit that includes this is built without contraction into FMAs.  Plain C++ outside hipcc.
//
// THE TIE RULE.  A cell's four winners are each the FIRST pixel, in the visiting order dx outer / dy inner (H:103-104), whose score is
// the cell's largest: every test is a strict > against a best that starts at 0 (H:100, :114-123), so a later pixel with an equal score
// and a pixel with a score of 0 never win.  With rank = dx * pot + dy that is the smallest rank among the largest positive scores.
#pragma once
#include "eds_init.hpp"

namespace edsini {

constexpr int32_t SPARSITY_START = 5;             // settings.cpp:212
constexpr int32_t SPARSITY_MAX = 1 << 30;         // where the reference's float-to-int conversion would be undefined, the value is this

// H:108-123: false where the pixel is below the gradient threshold; s = |dx|, |dy|, |dx - dy|, |dx + dy|
EDS_HD bool gms_scores(const Px& g, float THFac, float* s) {
    const float sqgd = g.dx * g.dx + g.dy * g.dy;
    const float TH = (THFac * 10.0f) * 0.75f;
    if (!(sqgd > TH * TH)) return false;
    s[0] = fabsf(g.dx); s[1] = fabsf(g.dy); s[2] = fabsf(g.dx - g.dy); s[3] = fabsf(g.dx + g.dy);
    return true;
}

// the cells of one axis: x = 1, 1 + pot, ... while x < w - pot (H:91-93)
EDS_HD int gms_cells(int w, int pot) { return w - pot > 1 ? (w - pot - 2) / pot + 1 : 0; }

// candidate (s, rank) against the held (bs, brank): the larger score, then the smaller rank; rank < 0 is "none", whose score is 0
EDS_HD bool gms_better(float s, int rank, float bs, int brank) { return s > bs || (s == bs && rank >= 0 && brank >= 0 && rank < brank); }

// gridMaxSelection (H:84-240; the templates 1 .. 11 and the generic form compute the same): map is w x h bytes, 0 / 1
inline int grid_max_selection(const Px* grads, uint8_t* map, int w, int h, int pot, float THFac) {
    memset(map, 0, (size_t)w * h);
    int numGood = 0;
    for (int y = 1; y < h - pot; y += pot)
        for (int x = 1; x < w - pot; x += pot) {
            int id[4] = {-1, -1, -1, -1};
            float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const Px* grads0 = grads + x + (size_t)y * w;
            for (int dx = 0; dx < pot; ++dx)
                for (int dy = 0; dy < pot; ++dy) {
                    const int idx = dx + dy * w;
                    float s[4];
                    if (!gms_scores(grads0[idx], THFac, s)) continue;
                    for (int k = 0; k < 4; ++k) if (s[k] > best[k]) { best[k] = s[k]; id[k] = idx; }
                }
            uint8_t* map0 = map + x + (size_t)y * w;
            for (int k = 0; k < 4; ++k)
                if (id[k] >= 0) {
                    if (!map0[id[k]]) numGood++;
                    map0[id[k]] = 1;
                }
        }
    return numGood;
}

// makePixelStatus's controller (H:243-297), the recursion as a loop.  pass(pot, THFac) runs one gridMaxSelection and returns numGood.
// *sparsity is the reference's global sparsityFactor: read, and left as the reference leaves it.  *passes: the passes that ran.
template <class Pass>
inline int make_pixel_status_ctl(Pass pass, float desiredDensity, int recsLeft, float THFac, int32_t* sparsity, int32_t* passes, int* err) {
    int32_t sp = *sparsity;
    int numGoodPoints = 0;
    *passes = 0;
    for (;;) {
        if (sp < 1) sp = 1;                                                     // H:245
        numGoodPoints = pass((int)sp, THFac, err);
        if (*err) return 0;
        ++*passes;
        const float quotia = numGoodPoints / (float)(desiredDensity);           // H:268
        const float grown = ((float)sp * sqrtf(quotia)) + 0.7f;                 // H:270
        int32_t newSparsity = grown < (float)SPARSITY_MAX ? (int32_t)grown : SPARSITY_MAX;
        if (newSparsity < 1) newSparsity = 1;
        const float oldTHFac = THFac;
        if (newSparsity == 1 && sp == 1) THFac = 0.5f;                          // H:277
        const int32_t diff = newSparsity > sp ? newSparsity - sp : sp - newSparsity;
        const bool stop = (diff < 1 && THFac == oldTHFac) || ((double)quotia > 0.8 && (double)(1.0f / quotia) > 0.8) || recsLeft == 0;   // H:280-282
        sp = newSparsity;
        if (stop) break;
        --recsLeft;
    }
    *sparsity = sp;
    return numGoodPoints;
}

inline int make_pixel_status(const Px* grads, uint8_t* map, int w, int h, float desiredDensity, int recsLeft, float THFac, int32_t* sparsity,
                             int32_t* passes) {
    int err = 0;
    return make_pixel_status_ctl([&](int pot, float th, int*) { return grid_max_selection(grads, map, w, h, pot, th); }, desiredDensity, recsLeft,
                                 THFac, sparsity, passes, &err);
}

}  // namespace edsini
