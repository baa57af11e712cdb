// DSO's pixel selector (include/eds_hip_select.h): what the device kernels (eds_pixsel.hip) and the host share — absSquaredGrad of
// makeImages, computeHistQuantil, makeHists, the per-pixel pieces of select cut the way the three kernels need them (the direction
// mask of a pot cell, the resolution of n2, the three arg-max keys of a pixel, what a 4 pot block writes) and the decisions of makeMaps
// — and a serial driver (make_maps_serial) that runs the same text, which the CPU tests compare with the literal numpy oracle.
// fp32 in the reference's order; every translation unit that includes this is built without contraction into FMAs.  Plain C++
// outside hipcc.  (csrc/eds_select.hpp, namespace edssel, is the radix select of the loss scale and has nothing to do with this.)
//
// Reference: src/mapping/PixelSelector.cpp (lines given per function), src/tracking/HessianBlocks.cpp:139-202 and
// HessianBlocks.h:384-390 for absSquaredGrad, src/utils/settings.cpp:145-148 for the four settings.
//
// THE n2 CHAIN.  select (:231-374) reads directions[randomPattern[n2] & 0xF] when it enters a 4 pot block, a 2 pot block and a pot cell,
// n2 being the number of level-0 selections of every cell visited before.  The cells are numbered in visiting order: 16 SLOTS per
// 4 pot block (blocks in raster order), slot = 4 * b3 + c2 with b3 the 2 pot block (raster inside the 4 pot block) and c2 the cell
// (raster inside the 2 pot block); a slot the image clips away has no pixel and never selects.
//   (a) cell_mask: bit d is set when the cell selects under direction d: some pixel has ag0 > th and dirNorm > 0 (:314-321, :349).
//   (b) a cell with mask 0x0000 or 0xFFFF is CERTAIN, any other AMBIGUOUS (a gradient exactly orthogonal to one of the directions).
//       n2 at a cell = (certain selecting cells before it) + (ambiguous cells before it that selected); the ambiguous cells are
//       resolved in order with cell_selected(mask, table, n2).  Exact for any input, serial in the ambiguous cells only.
//   (c) pixel_keys / finish_block: a level-0 improvement sets bestIdx3 = bestIdx4 = -2 for good and a level-1 improvement bestIdx4 = -2,
//       so a 2 pot block selects at level 1 exactly when none of its cells selected, and then over ALL its pixels; a 4 pot block
//       selects at level 2 exactly when none of its cells and none of its 2 pot blocks selected.  `dirNorm > bestVal` with bestVal
//       starting at 0 and a strict > is the FIRST pixel in visiting order among those of the largest dirNorm > 0: the arg-max of the
//       key (dirNorm, -visiting order).  bestIdx > 0 always holds for a winner: the border rule excludes pixel 0.
//
// Quirks kept: the bounds xf < 4 || xf >= w - 5 || yf < 4 || yf > h - 4 (:305); pixelTH2 = pixelTH1 * dw2 with dw2 = dw1 * dw1, which is
// dw1^3 (:270-271, :310); the level-1 pixel (int)(xf * 0.5f + 0.25f), the level-2 pixel (int)(xf * 0.25f + 0.125) (:325, :337); the 16
// directions are the double literals narrowed to float (:248-264); dirNorm = fabsf(gx * dx + gy * dy), left to right; only the
// w / 32 x h / 32 full blocks are histogrammed, border skip it > w - 2 || jt > h - 2 || it < 1 || jt < 1 (:84-100); the smoothing sums
// column x - 1 at (y - 1, y + 1, y), column x + 1, then (x, y - 1), (x, y + 1), (x, y), result (sum / num) * (sum / num) (:105-129);
// computeHistQuantil's th = (int)(hist[0] * below + 0.5f) with the product in fp32 (:60-69); makeMaps' float expressions as written
// (:136-227): quotia = numWant / numHave, K = (numHave * (pot + 1)) * (pot + 1), idealPotential = (int)(sqrtf(K / numWant) - 1),
// charTH = (unsigned char)(255 * quotia), rn advancing once per non-zero pixel in flat order; the comparisons of quotia with
// 1.25, 0.25 and 0.95 are fp64 comparisons of the widened float, as C++ makes them.
//
// DEFINED BEHAVIOUR where the reference is undefined:
//  1. thsSmoothed[(xf >> 5) + (yf >> 5) * thsStep] with W or H no multiple of 32: the flat index as it is while it is below
//     w32 * h32 (it then aliases the next block row's first entry, as in the reference); otherwise, where the reference reads
//     uninitialised memory, the block (min(xf >> 5, w32 - 1), min(yf >> 5, h32 - 1)).  ths_index().
//  2. (int)sqrtf(v) is 48 when the root is NaN or not below 49: no non-finite float is converted.  Comparisons with a NaN
//     absSquaredGrad are false, as in the reference.  hist_bin().
//  3. numHave == 0 gives quotia = +inf; the float rules decide as written; idealPotential is 1 when sqrtf(K / numWant) - 1 is NaN or
//     below 1 and 2^30 when it is not below 2^30: no integer is formed from a non-finite float.  decide().
//  4. Any potential 1 .. 2^30 is accepted; a potential above max(W, H) selects as max(W, H) does (one cell holds the image), and a
//     4 pot block larger than the image is one block.
//  5. computeHistQuantil reads hist[1 .. 90] of an array of which makeHists zeroes 50 entries: bins 50 .. 90 are 0 here.  The gamma
//     weight's (int)(colour + 0.5f) is 5 when the sum is NaN or below 5 and 250 when it is not below 250, which is the reference's
//     clamp for every finite colour.  absSquaredGrad of rows 0 and h - 1, which the reference leaves uninitialised and never
//     reads, is 0.  The table index n2 is always below the number of selected cells, which is below W H.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cstdlib>
#include <vector>

#include "eds_dso_common.hpp"

namespace edspix {

using edsdso::Px;                                  // {c, dx, dy, pad}: pad holds absSquaredGrad here
typedef unsigned long long Key;

constexpr int LEVELS = 3;
constexpr int SLOTS = 16;                          // cells per 4 pot block
constexpr int MAX_POTENTIAL = 1 << 30;
constexpr int MAX_SIDE = 8192;                     // 16 * MAX_SIDE^2 visiting ranks fit 31 bits

// eds_sel_params, member for member (settings.cpp:145-148)
struct Params {
    float min_grad_hist_cut, min_grad_hist_add, grad_downweight_per_level;
    int32_t select_direction_distribution;
};

struct Geo { int32_t w, h, w1, h1, w2, h2, w32, h32; };

struct Pass { int32_t potential, n2, n3, n4; };    // eds_sel_pass

EDS_HD Params params_default() { Params p = {0.5f, 7.0f, 0.75f, 1}; return p; }
EDS_HD bool params_valid(const Params& p) {
    return edsdso::finite_f(p.min_grad_hist_cut) && edsdso::finite_f(p.min_grad_hist_add) && edsdso::finite_f(p.grad_downweight_per_level) &&
           p.min_grad_hist_cut >= 0.0f && p.min_grad_hist_cut <= 1.0f;
}

EDS_HD Geo make_geo(int H, int W) {
    Geo g = {W, H, W >> 1, H >> 1, W >> 2, H >> 2, W / 32, H / 32};
    return g;
}
EDS_HD int level_w(const Geo& g, int l) { return l == 0 ? g.w : l == 1 ? g.w1 : g.w2; }
EDS_HD int level_h(const Geo& g, int l) { return l == 0 ? g.h : l == 1 ? g.h1 : g.h2; }

// ---- makeImages: absSquaredGrad (HessianBlocks.cpp:193-199, getBGradOnly HessianBlocks.h:384-390) -------------------------------------
EDS_HD int gamma_index(float colour) {
    const float t = colour + 0.5f;
    if (!(t >= 5.0f)) return 5;
    if (!(t < 250.0f)) return 250;
    return (int)t;
}
// B: the 256 floats of CalibHessian::B, or NULL for HCalib == 0
EDS_HD float abs_grad(float dx, float dy, float colour, const float* B) {
    float dabs = dx * dx + dy * dy;
    if (B) {
        const int c = gamma_index(colour);
        const float gw = B[c + 1] - B[c];
        dabs *= gw * gw;
    }
    return dabs;
}
// one pixel of a level after its colours are there: dx, dy by edsdso's restatement, absSquaredGrad into pad
EDS_HD void gradient_pixel(Px* p, int w, int h, int i, const float* B) {
    float dx, dy;
    edsdso::gradient_at(p, w, h, i, &dx, &dy);
    p[i].dx = dx; p[i].dy = dy;
    p[i].pad = edsdso::border_row(w, h, i) ? 0.0f : abs_grad(dx, dy, p[i].c, B);
}

// ---- computeHistQuantil, makeHists (:60-135) ------------------------------------------------------------------------------------------
EDS_HD bool hist_counted(int it, int jt, int w, int h) { return !(it > w - 2 || jt > h - 2 || it < 1 || jt < 1); }
EDS_HD int hist_bin(float v) {
    const float r = sqrtf(v);
    if (!(r < 49.0f)) return 48;
    const int g = (int)r;
    return g > 48 ? 48 : g;
}
// hist[0]: the number of pixels; hist[1 + g]: those of bin g, g = 0 .. 48
EDS_HD int hist_quantile(const int* hist, float below) {
    int th = (int)(hist[0] * below + 0.5f);
    for (int i = 0; i < 90; ++i) {
        if (i + 1 < 50) th -= hist[i + 1];
        if (th < 0) return i;
    }
    return 90;
}
EDS_HD float block_threshold(const int* hist, const Params& s) { return hist_quantile(hist, s.min_grad_hist_cut) + s.min_grad_hist_add; }

EDS_HD float smooth_at(const float* ths, int w32, int h32, int x, int y) {
    float sum = 0, num = 0;
    if (x > 0) {
        if (y > 0) { num++; sum += ths[x - 1 + (y - 1) * w32]; }
        if (y < h32 - 1) { num++; sum += ths[x - 1 + (y + 1) * w32]; }
        num++; sum += ths[x - 1 + y * w32];
    }
    if (x < w32 - 1) {
        if (y > 0) { num++; sum += ths[x + 1 + (y - 1) * w32]; }
        if (y < h32 - 1) { num++; sum += ths[x + 1 + (y + 1) * w32]; }
        num++; sum += ths[x + 1 + y * w32];
    }
    if (y > 0) { num++; sum += ths[x + (y - 1) * w32]; }
    if (y < h32 - 1) { num++; sum += ths[x + (y + 1) * w32]; }
    num++; sum += ths[x + y * w32];
    return (sum / num) * (sum / num);
}

// defined behaviour 1
EDS_HD int ths_index(int xf, int yf, int w32, int h32) {
    const int bx = xf >> 5, by = yf >> 5, flat = bx + by * w32;
    if (flat < w32 * h32) return flat;
    return (bx < w32 - 1 ? bx : w32 - 1) + (by < h32 - 1 ? by : h32 - 1) * w32;
}

// ---- select (:231-374) ----------------------------------------------------------------------------------------------------------------
EDS_HD float dir_x(int i) {
    const float t[16] = {(float)0, (float)0.3827, (float)0.1951, (float)0.9239, (float)0.7071, (float)0.3827, (float)0.8315, (float)0.8315,
                         (float)0.5556, (float)0.9808, (float)0.9239, (float)0.7071, (float)0.5556, (float)0.9808, (float)1.0000, (float)0.1951};
    return t[i];
}
EDS_HD float dir_y(int i) {
    const float t[16] = {(float)1.0000, (float)0.9239, (float)0.9808, (float)0.3827, (float)0.7071, (float)-0.9239, (float)0.5556, (float)-0.5556,
                         (float)-0.8315, (float)0.1951, (float)-0.3827, (float)-0.7071, (float)0.8315, (float)-0.1951, (float)0.0000, (float)-0.9808};
    return t[i];
}

// what one select pass reads
struct Sel {
    const Px *l0, *l1, *l2;
    const float* ths_s;                            // thsSmoothed[w32 * h32]
    Geo g;
    float dw1, dw2, thf;
    int32_t dist;                                  // setting_selectDirectionDistribution
    int32_t pot;                                   // min(potential, max(w, h)): defined behaviour 4
    int32_t nbx, nby;                              // 4 pot blocks per row and column
};

EDS_HD Sel make_sel(const Px* l0, const Px* l1, const Px* l2, const float* ths_s, const Geo& g, const Params& s, float thf, int potential) {
    Sel S;
    S.l0 = l0; S.l1 = l1; S.l2 = l2; S.ths_s = ths_s; S.g = g;
    S.dw1 = s.grad_downweight_per_level;
    S.dw2 = S.dw1 * S.dw1;
    S.thf = thf;
    S.dist = s.select_direction_distribution;
    const int side = g.w > g.h ? g.w : g.h;
    S.pot = potential < side ? potential : side;
    S.nbx = (g.w + 4 * S.pot - 1) / (4 * S.pot);
    S.nby = (g.h + 4 * S.pot - 1) / (4 * S.pot);
    return S;
}

EDS_HD bool pixel_in(int xf, int yf, int w, int h) { return !(xf < 4 || xf >= w - 5 || yf < 4 || yf > h - 4); }

// a pot cell: origin and extent; mx < 1 or my < 1: the image clips it away
struct Cell { int x0, y0, mx, my; };
EDS_HD int min_i(int a, int b) { return a < b ? a : b; }
EDS_HD Cell cell_of(const Sel& S, int b4, int slot) {
    const int p = S.pot, w = S.g.w, h = S.g.h;
    const int x4 = (b4 % S.nbx) * 4 * p, y4 = (b4 / S.nbx) * 4 * p;
    const int b3 = slot >> 2, c2 = slot & 3;
    Cell c = {0, 0, 0, 0};
    const int x3 = (b3 & 1) * 2 * p, y3 = (b3 >> 1) * 2 * p;
    if (x3 >= min_i(4 * p, w - x4) || y3 >= min_i(4 * p, h - y4)) return c;
    const int x34 = x3 + x4, y34 = y3 + y4, x2 = (c2 & 1) * p, y2 = (c2 >> 1) * p;
    if (x2 >= min_i(2 * p, w - x34) || y2 >= min_i(2 * p, h - y34)) return c;
    c.x0 = x2 + x34; c.y0 = y2 + y34;
    c.mx = min_i(p, w - c.x0); c.my = min_i(p, h - c.y0);
    return c;
}

EDS_HD float dir_norm(const Px& q, int d) { return fabsf(q.dx * dir_x(d) + q.dy * dir_y(d)); }

// (a) the directions under which the level-0 pixel (xf, yf) makes its cell select
EDS_HD unsigned pixel_mask(const Sel& S, int xf, int yf) {
    if (!pixel_in(xf, yf, S.g.w, S.g.h)) return 0u;
    const float pixelTH0 = S.ths_s[ths_index(xf, yf, S.g.w32, S.g.h32)];
    const Px q = S.l0[xf + S.g.w * yf];
    const float ag0 = q.pad;
    if (!(ag0 > pixelTH0 * S.thf)) return 0u;
    if (!S.dist) return ag0 > 0.0f ? 0xFFFFu : 0u;
    unsigned m = 0u;
    for (int d = 0; d < 16; ++d)
        if (dir_norm(q, d) > 0.0f) m |= 1u << d;
    return m;
}
EDS_HD unsigned cell_mask(const Sel& S, const Cell& c) {
    unsigned m = 0u;
    for (int y = 0; y < c.my; ++y)
        for (int x = 0; x < c.mx; ++x) m |= pixel_mask(S, c.x0 + x, c.y0 + y);
    return m;
}

// (b)
EDS_HD bool mask_certain(unsigned m) { return m == 0u || m == 0xFFFFu; }
EDS_HD int table_dir(const uint8_t* table, int n2, int wh) { return table[n2 < wh ? n2 : wh - 1] & 0xF; }
EDS_HD int cell_selected(unsigned mask, const uint8_t* table, int n2, int wh) { return (int)((mask >> table_dir(table, n2, wh)) & 1u); }

// (c) what a 4 pot block knows when its pixels are read: which cells select, and the directions drawn at the three levels
struct Block {
    int32_t x4, y4, bw, bh;
    uint32_t sel;                                  // bit slot: the cell selects at level 0
    uint8_t d2[SLOTS], d3[4], d4;
};
EDS_HD void make_block(const Sel& S, int b4, const int32_t* n2_start, const uint8_t* cell_sel, const uint8_t* table, Block& B) {
    const int p = S.pot, wh = S.g.w * S.g.h;
    B.x4 = (b4 % S.nbx) * 4 * p; B.y4 = (b4 / S.nbx) * 4 * p;
    B.bw = min_i(4 * p, S.g.w - B.x4); B.bh = min_i(4 * p, S.g.h - B.y4);
    B.sel = 0u;
    for (int s = 0; s < SLOTS; ++s) {
        if (cell_sel[s]) B.sel |= 1u << s;
        B.d2[s] = (uint8_t)table_dir(table, n2_start[s], wh);
    }
    for (int b = 0; b < 4; ++b) B.d3[b] = B.d2[4 * b];
    B.d4 = B.d2[0];
}
EDS_HD bool block3_hit(const Block& B, int b3) { return ((B.sel >> (4 * b3)) & 0xFu) != 0u; }

EDS_HD uint32_t float_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
// v > 0 (+inf included): larger v, then the earlier visiting rank, is the larger key; 0 is "no candidate"
EDS_HD Key make_key(float v, uint32_t ord) { return ((Key)float_bits(v) << 32) | (Key)(0xFFFFFFFFu - ord); }
EDS_HD uint32_t key_ord(Key k) { return 0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull); }

// the pixel (lx, ly) of block B: its slot and its three keys (0: it does not compete at that level)
EDS_HD int pixel_keys(const Sel& S, const Block& B, int lx, int ly, Key* k2, Key* k3, Key* k4) {
    const int p = S.pot;
    const int b3 = ((ly >= 2 * p) << 1) | (lx >= 2 * p);
    const int rx = lx - (b3 & 1) * 2 * p, ry = ly - (b3 >> 1) * 2 * p;
    const int c2 = ((ry >= p) << 1) | (rx >= p);
    const int x1 = rx - (c2 & 1) * p, y1 = ry - (c2 >> 1) * p;
    const int slot = 4 * b3 + c2;
    *k2 = 0; *k3 = 0; *k4 = 0;
    const int xf = B.x4 + lx, yf = B.y4 + ly, w = S.g.w;
    if (!pixel_in(xf, yf, w, S.g.h)) return slot;
    const uint32_t ord = ((uint32_t)slot * (uint32_t)p + (uint32_t)y1) * (uint32_t)p + (uint32_t)x1;
    const float pixelTH0 = S.ths_s[ths_index(xf, yf, S.g.w32, S.g.h32)];
    const float pixelTH1 = pixelTH0 * S.dw1;
    const float pixelTH2 = pixelTH1 * S.dw2;
    const Px q = S.l0[xf + w * yf];
    if ((B.sel >> slot) & 1u) {
        const float ag0 = q.pad;
        if (ag0 > pixelTH0 * S.thf) {
            const float dirNorm = S.dist ? dir_norm(q, B.d2[slot]) : ag0;
            if (dirNorm > 0.0f) *k2 = make_key(dirNorm, ord);
        }
    }
    if (block3_hit(B, b3)) return slot;
    const float ag1 = S.l1[(int)(xf * 0.5f + 0.25f) + (int)(yf * 0.5f + 0.25f) * S.g.w1].pad;
    if (ag1 > pixelTH1 * S.thf) {
        const float dirNorm = S.dist ? dir_norm(q, B.d3[b3]) : ag1;
        if (dirNorm > 0.0f) *k3 = make_key(dirNorm, ord);
    }
    if (B.sel) return slot;
    const float ag2 = S.l2[(int)(xf * 0.25f + 0.125) + (int)(yf * 0.25f + 0.125) * S.g.w2].pad;
    if (ag2 > pixelTH2 * S.thf) {
        const float dirNorm = S.dist ? dir_norm(q, B.d4) : ag2;
        if (dirNorm > 0.0f) *k4 = make_key(dirNorm, ord);
    }
    return slot;
}

// the flat index of the pixel a key names
EDS_HD int key_pixel(const Sel& S, const Block& B, Key k) {
    const uint32_t ord = key_ord(k), p = (uint32_t)S.pot;
    const int x1 = (int)(ord % p), y1 = (int)((ord / p) % p), slot = (int)(ord / p / p);
    const int b3 = slot >> 2, c2 = slot & 3;
    const int xf = B.x4 + (b3 & 1) * 2 * S.pot + (c2 & 1) * S.pot + x1, yf = B.y4 + (b3 >> 1) * 2 * S.pot + (c2 >> 1) * S.pot + y1;
    return xf + S.g.w * yf;
}

// what item `item` of a block's 21 writes: 0 .. 15 a cell (map value 1), 16 .. 19 a 2 pot block (2), 20 the 4 pot block (4).
// K2[16], K3[4], K4[1] are the arg-max keys.  Returns the map value written, 0 for none.
EDS_HD int finish_item(const Sel& S, const Block& B, const Key* K2, const Key* K3, const Key* K4, int item, uint8_t* map) {
    if (item < SLOTS) {
        if (!((B.sel >> item) & 1u) || K2[item] == 0) return 0;
        map[key_pixel(S, B, K2[item])] = 1;
        return 1;
    }
    if (item < SLOTS + 4) {
        const int b3 = item - SLOTS;
        if (block3_hit(B, b3) || K3[b3] == 0) return 0;
        map[key_pixel(S, B, K3[b3])] = 2;
        return 2;
    }
    if (B.sel || K4[0] == 0) return 0;
    for (int b3 = 0; b3 < 4; ++b3)
        if (K3[b3] != 0) return 0;                 // (no cell selected, so every K3 is a level-1 selection)
    map[key_pixel(S, B, K4[0])] = 4;
    return 4;
}

// ---- makeMaps (:136-227): what follows a select pass -----------------------------------------------------------------------------------
struct Decision {
    int32_t recurse;                               // 1: select again at new_potential
    int32_t new_potential;                         // currentPotential after this step
    int32_t subselect;                             // 1: quotia < 0.95
    int32_t char_th;
    float quotia;
};
EDS_HD Decision decide(int n2, int n3, int n4, float density, int recursionsLeft, int currentPotential) {
    Decision D;
    const float numHave = (float)(n2 + n3 + n4);
    const float numWant = density;
    const float quotia = numWant / numHave;
    const float K = numHave * (currentPotential + 1) * (currentPotential + 1);
    const float f = sqrtf(K / numWant) - 1;
    int idealPotential = !(f >= 1.0f) ? 1 : !(f < 1073741824.0f) ? MAX_POTENTIAL : (int)f;
    if (idealPotential < 1) idealPotential = 1;
    D.quotia = quotia; D.recurse = 0; D.subselect = 0; D.char_th = 0;
    if (recursionsLeft > 0 && (double)quotia > 1.25 && currentPotential > 1) {
        if (idealPotential >= currentPotential) idealPotential = currentPotential - 1;
        D.recurse = 1;
    } else if (recursionsLeft > 0 && (double)quotia < 0.25) {
        if (idealPotential <= currentPotential) idealPotential = currentPotential < MAX_POTENTIAL ? currentPotential + 1 : MAX_POTENTIAL;
        D.recurse = 1;
    }
    D.new_potential = idealPotential;
    if (!D.recurse && (double)quotia < 0.95) {
        D.subselect = 1;
        D.char_th = (int)(unsigned char)(int)(255 * quotia);
    }
    return D;
}
// the sub-selection's rule for the non-zero pixel of rank rn
EDS_HD bool sub_removed(const uint8_t* table, int rn, int char_th) { return (int)table[rn] > char_th; }

// ---- the serial driver (host only) -----------------------------------------------------------------------------------------------------------------
// the constructor's table (:37-39).  Reseeds the C library's generator.
inline void fill_reference_pattern(uint8_t* out, size_t n) {
    srand(3141592);
    for (size_t i = 0; i < n; ++i) out[i] = (uint8_t)(rand() & 0xFF);
}

struct Serial {
    Geo g;
    Params prm;
    int potential = 3;
    bool hist_valid = false;
    std::vector<Px> lv[LEVELS];
    std::vector<float> ths, ths_s;
    std::vector<uint8_t> map, table;
    std::vector<uint32_t> mask;                    // of the last select pass, per slot
    std::vector<int32_t> n2_start;
    std::vector<uint8_t> cell_sel;
    int ambiguous = 0;                             // ambiguous cells of the last select pass
    int n2_certain = 0;                            // what n2 would be from the certain cells alone
};

inline void serial_init(Serial& s, int H, int W) {
    s.g = make_geo(H, W);
    s.prm = params_default();
    s.potential = 3;
    s.hist_valid = false;
    for (int l = 0; l < LEVELS; ++l) s.lv[l].assign((size_t)level_w(s.g, l) * level_h(s.g, l), Px{0, 0, 0, 0});
    s.ths.assign((size_t)s.g.w32 * s.g.h32, 0.0f);
    s.ths_s = s.ths;
    s.map.assign((size_t)W * H, 0);
}

inline void serial_set_image(Serial& s, const float* image, int64_t row_stride, const float* B) {
    Px* lv[LEVELS] = {s.lv[0].data(), s.lv[1].data(), s.lv[2].data()};
    edsdso::make_levels(image, row_stride, s.g.w, s.g.h, LEVELS, lv);
    for (int l = 0; l < LEVELS; ++l)
        for (int i = 0; i < level_w(s.g, l) * level_h(s.g, l); ++i) gradient_pixel(lv[l], level_w(s.g, l), level_h(s.g, l), i, B);
    s.hist_valid = false;
}

inline void serial_make_hists(Serial& s) {
    const Geo& g = s.g;
    for (int y = 0; y < g.h32; ++y)
        for (int x = 0; x < g.w32; ++x) {
            int hist[50] = {0};
            for (int j = 0; j < 32; ++j)
                for (int i = 0; i < 32; ++i) {
                    const int it = i + 32 * x, jt = j + 32 * y;
                    if (!hist_counted(it, jt, g.w, g.h)) continue;
                    hist[hist_bin(s.lv[0][it + jt * g.w].pad) + 1]++;
                    hist[0]++;
                }
            s.ths[x + y * g.w32] = block_threshold(hist, s.prm);
        }
    for (int y = 0; y < g.h32; ++y)
        for (int x = 0; x < g.w32; ++x) s.ths_s[x + y * g.w32] = smooth_at(s.ths.data(), g.w32, g.h32, x, y);
    s.hist_valid = true;
}

// select in the form (a) - (c); n[3] = n2, n3, n4
inline void serial_select(Serial& s, int potential, float thf, int n[3]) {
    const Sel S = make_sel(s.lv[0].data(), s.lv[1].data(), s.lv[2].data(), s.ths_s.data(), s.g, s.prm, thf, potential);
    const int nb = S.nbx * S.nby, ns = nb * SLOTS, wh = s.g.w * s.g.h;
    s.mask.assign((size_t)ns, 0u);
    s.n2_start.assign((size_t)ns, 0);
    s.cell_sel.assign((size_t)ns, 0);
    for (int i = 0; i < ns; ++i) s.mask[i] = cell_mask(S, cell_of(S, i / SLOTS, i % SLOTS));
    // the prefix sum over the certain cells, then the ambiguous cells in order
    std::vector<int32_t> P((size_t)ns), A((size_t)ns), amb;
    int certain = 0;
    for (int i = 0; i < ns; ++i) {
        P[i] = certain; A[i] = (int32_t)amb.size();
        if (s.mask[i] == 0xFFFFu) ++certain;
        else if (!mask_certain(s.mask[i])) amb.push_back(i);
    }
    std::vector<int32_t> extra(amb.size() + 1, 0);
    for (size_t k = 0; k < amb.size(); ++k)
        extra[k + 1] = extra[k] + cell_selected(s.mask[amb[k]], s.table.data(), P[amb[k]] + extra[k], wh);
    for (int i = 0; i < ns; ++i) {
        s.n2_start[i] = P[i] + extra[A[i]];
        s.cell_sel[i] = (uint8_t)cell_selected(s.mask[i], s.table.data(), s.n2_start[i], wh);
    }
    s.ambiguous = (int)amb.size();
    s.n2_certain = certain;
    n[0] = certain + extra[amb.size()]; n[1] = 0; n[2] = 0;
    s.map.assign((size_t)wh, 0);
    for (int b4 = 0; b4 < nb; ++b4) {
        Block B;
        make_block(S, b4, &s.n2_start[(size_t)b4 * SLOTS], &s.cell_sel[(size_t)b4 * SLOTS], s.table.data(), B);
        Key K[SLOTS + 5] = {0};
        for (int ly = 0; ly < B.bh; ++ly)
            for (int lx = 0; lx < B.bw; ++lx) {
                Key k2, k3, k4;
                const int slot = pixel_keys(S, B, lx, ly, &k2, &k3, &k4);
                if (k2 > K[slot]) K[slot] = k2;
                if (k3 > K[SLOTS + (slot >> 2)]) K[SLOTS + (slot >> 2)] = k3;
                if (k4 > K[SLOTS + 4]) K[SLOTS + 4] = k4;
            }
        for (int item = 0; item < SLOTS + 5; ++item) {
            const int v = finish_item(S, B, K, K + SLOTS, K + SLOTS + 4, item, s.map.data());
            if (v == 2) ++n[1];
            if (v == 4) ++n[2];
        }
    }
}

// makeMaps whole; passes (and pass_maps, the map after every select pass) may be NULL.  Returns numHaveSub, -1 without a table.
inline int make_maps_serial(Serial& s, float density, int recursions_left, float th_factor, std::vector<Pass>* passes,
                            std::vector<std::vector<uint8_t>>* pass_maps) {
    if (s.table.size() != s.map.size()) return -1;
    if (!s.hist_valid) serial_make_hists(s);
    for (;;) {
        int n[3];
        serial_select(s, s.potential, th_factor, n);
        if (passes) passes->push_back(Pass{s.potential, n[0], n[1], n[2]});
        if (pass_maps) pass_maps->push_back(s.map);
        const Decision D = decide(n[0], n[1], n[2], density, recursions_left, s.potential);
        s.potential = D.new_potential;
        if (D.recurse) { --recursions_left; continue; }
        int numHaveSub = n[0] + n[1] + n[2];
        if (D.subselect) {
            int rn = 0;
            for (size_t i = 0; i < s.map.size(); ++i)
                if (s.map[i] != 0) {
                    if (sub_removed(s.table.data(), rn, D.char_th)) { s.map[i] = 0; --numHaveSub; }
                    ++rn;
                }
        }
        return numHaveSub;
    }
}

// the map's non-zero pixels in row-major order
inline int selection_serial(const Serial& s, std::vector<int32_t>& uv, std::vector<float>& type) {
    uv.clear(); type.clear();
    for (int i = 0; i < (int)s.map.size(); ++i)
        if (s.map[i]) { uv.push_back(i % s.g.w); uv.push_back(i / s.g.w); type.push_back((float)s.map[i]); }
    return (int)type.size();
}

}  // namespace edspix
