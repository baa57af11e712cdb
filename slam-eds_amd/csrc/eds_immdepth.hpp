// Immature points seeded from a depth map (include/eds_hip_immdepth.h): the loop that drives ImmaturePoint's second constructor, one
// pixel at a time, over the pinned k-d walk (eds_kdtree.hpp) and the constructor (eds_immature.hpp).  What the device kernels
// (eds_immdepth.hip) and the host run is this code; the CPU tests compare it with a numpy statement of the same loop.  fp64 without
// contraction into FMAs for the query, the walk and the distance, fp32 for the constructor.  Plain C++ outside hipcc.
//
// For the pixel (u, v) and a map of m points given in tree order (txy, tidp, perm: position -> the caller's index):
//   q = ((double)u * scale[0], (double)v * scale[1]);   k = nnSearch(q)  (edskd::nn: strict <, near side first, the first point of the
//   traversal wins an exact tie);   idepth = (float)tidp[k];   dx = txy[k].x - (double)u, dy = txy[k].y - (double)v against the
//   UNSCALED pixel, distance = sqrt(dx * dx + dy * dy);   then the second constructor.  m = 0: the first constructor.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "eds_immature.hpp"
#include "eds_kdtree.hpp"

namespace edsimd {

// what a pixel took from the map: position in tree order (-1: the map is empty), the caller's index, and the constructor's two inputs
struct Nearest {
    int32_t pos, index;
    float idepth;
    double distance;
};

EDS_HD Nearest none() {
    Nearest r;
    r.pos = -1; r.index = -1; r.idepth = 0.0f; r.distance = 0.0;
    return r;
}

EDS_HD void query_of(int u, int v, double sx, double sy, double* qx, double* qy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    *qx = (double)u * sx;
    *qy = (double)v * sy;
}

// steps 3 and 4 for the walk's winner k; tx, ty: its coordinates
EDS_HD Nearest winner(int k, double tx, double ty, const double* tidp, const int32_t* perm, int u, int v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    Nearest r;
    r.pos = k;
    r.index = perm[k];
    r.idepth = (float)tidp[k];
    const double dx = tx - (double)u, dy = ty - (double)v;
    r.distance = sqrt(dx * dx + dy * dy);
    return r;
}

// steps 1 to 4 on the tree in ordinary memory: the simple form of the walk
EDS_HD Nearest nearest(const double* txy, const double* tidp, const int32_t* perm, int m, int u, int v, double sx, double sy) {
    if (m < 1) return none();
    double qx, qy;
    query_of(u, v, sx, sy, &qx, &qy);
    const int k = edskd::nn(txy, m, qx, qy, nullptr);
    return winner(k, txy[2 * (size_t)k], txy[2 * (size_t)k + 1], tidp, perm, u, v);
}

// step 5
EDS_HD void construct(edsimm::Point& p, const float* c, int W, int H, const edsimm::Params& s, int u, int v, float type, const Nearest& nn) {
    edsimm::construct(p, c, W, H, s, u, v, type, nn.pos >= 0, nn.idepth, nn.distance);
}

// the whole loop body
EDS_HD Nearest seed(edsimm::Point& p, const float* c, int W, int H, const edsimm::Params& s, int u, int v, float type, const double* txy,
                    const double* tidp, const int32_t* perm, int m, double sx, double sy) {
    const Nearest nn = nearest(txy, tidp, perm, m, u, v, sx, sy);
    construct(p, c, W, H, s, u, v, type, nn);
    return nn;
}

// a non-finite coordinate in a map of n points
inline bool map_finite(const double* xy, int n) {
    for (size_t i = 0; i < 2 * (size_t)n; ++i) if (!(fabs(xy[i]) <= 1.79769313486231570815e+308)) return false;
    return true;
}

}  // namespace edsimd
