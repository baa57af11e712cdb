// The shared sparse splat and blur (slam-eds_amd/csrc/eds_splat.hpp) on the host, bit for bit against a dense restatement of
// drawValuesPoints (reference src/utils/Utils.cpp:124-193): one loop over the points in index order that adds the four corner weights
// into an image, then the 3 x 3 Gaussian blur.  Frames 5 x 7 and 1 x 4, 40 points, key bias 0 (the KLT's) and 1 (the epiline
// model's), one fp64 value plane (the epiline's instantiation) and two fp32 planes (the KLT's).  Also the two reflect-101 spellings
// the trackers used to carry.  Build with -ffp-contract=off; exit status 0 = every pixel equal.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../slam-eds_amd/csrc/eds_splat.hpp"

using namespace edssplat;

namespace {

const int NPTS = 40;

struct Lcg {
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }   // [0, 1)
};

int clipi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
int mirror(int p, int len) { return len == 1 ? 0 : (p < 0 ? -p : (p >= len ? 2 * len - 2 - p : p)); }      // one reflection: p in [-1, len]

// which points get a key: bias 0 as getCoord(true) leaves them (0 <= x <= W, 0 <= y <= H), bias 1 every footprint that touches the image
bool keyed(double x, double y, int W, int H, int bias) {
    return bias ? (x > -1.0 && x < (double)W && y > -1.0 && y < (double)H) : (x >= 0.0 && x <= (double)W && y >= 0.0 && y <= (double)H);
}

// 40 points: generic fractions (so that the order of a sum shows in its last bit), exact integers, repeated coordinates, the frame's
// far edge, points without a key; bias 1 adds x or y in (-1, 0) and x = W - 0.5
std::vector<double> make_points(int H, int W, int bias, Lcg& rng) {
    std::vector<double> c(2 * NPTS);
    for (int i = 0; i < NPTS; ++i) {
        double x = bias ? rng.next() * (W + 1) - 1.0 : rng.next() * W, y = bias ? rng.next() * (H + 1) - 1.0 : rng.next() * H;
        switch (i % 10) {
            case 1: x = (double)(i % W); y = (double)(i % H); break;                    // exact integers
            case 2: x = c[2 * (i - 2)]; y = c[2 * (i - 2) + 1]; break;                  // a repeated generic point
            case 3: x = c[2 * (i - 2)]; y = c[2 * (i - 2) + 1]; break;                  // a repeated integer point
            case 4: x = bias ? -0.25 - 0.5 * rng.next() : 0.0; break;                   // x in (-1, 0) / on the left edge
            case 5: y = bias ? -0.25 - 0.5 * rng.next() : (double)H; break;             // y in (-1, 0) / y = H
            case 6: x = W - 0.5; break;
            case 7: x = bias ? -1.0 : W + 0.5; break;                                   // no key
            case 8: x = bias ? -0.5 : (double)W; y = bias ? -0.5 : y; break;            // both in (-1, 0) / x = W
            default: break;
        }
        c[2 * i] = x; c[2 * i + 1] = y;
    }
    return c;
}

// the dense restatement: every point adds its four weighted corners in index order, a corner outside the frame with weight 0 on the
// clipped pixel; then rows, then columns of [k0 k1 k0] on mirrored neighbours
std::vector<double> dense(int H, int W, const std::vector<double>& c, const std::vector<double>& val, double k0, double k1) {
    std::vector<double> img((size_t)H * W, 0.0), row((size_t)H * W), out((size_t)H * W);
    for (int i = 0; i < NPTS; ++i) {
        const double x = c[2 * i], y = c[2 * i + 1], v = val[i];
        const int xa = (int)floor(x), ya = (int)floor(y), xb = xa + 1, yb = ya + 1;
        const bool xa_in = xa >= 0 && xa < W, xb_in = xb >= 0 && xb < W, ya_in = ya >= 0 && ya < H, yb_in = yb >= 0 && yb < H;
        const double w_aa = xa_in && ya_in ? (xb - x) * (yb - y) : 0.0, w_ab = xa_in && yb_in ? (xb - x) * (y - ya) : 0.0;
        const double w_ba = xb_in && ya_in ? (x - xa) * (yb - y) : 0.0, w_bb = xb_in && yb_in ? (x - xa) * (y - ya) : 0.0;
        const int cxa = clipi(xa, W - 1), cxb = clipi(xb, W - 1), cya = clipi(ya, H - 1), cyb = clipi(yb, H - 1);
        img[cya * W + cxa] += w_aa * v;
        img[cyb * W + cxa] += w_ab * v;
        img[cya * W + cxb] += w_ba * v;
        img[cyb * W + cxb] += w_bb * v;
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            row[y * W + x] = k0 * img[y * W + mirror(x - 1, W)] + k1 * img[y * W + x] + k0 * img[y * W + mirror(x + 1, W)];
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            out[y * W + x] = k0 * row[mirror(y - 1, H) * W + x] + k1 * row[y * W + x] + k0 * row[mirror(y + 1, H) * W + x];
    return out;
}

template <int NV, typename T>
int check(int H, int W, int bias, Lcg& rng) {
    const std::vector<double> c = make_points(H, W, bias, rng);
    std::vector<T> planes[NV];
    const T* V[NV];
    for (int v = 0; v < NV; ++v) {
        for (int i = 0; i < NPTS; ++i) planes[v].push_back((T)(rng.next() * 2.0 - 1.0) / (T)3);
        V[v] = planes[v].data();
    }
    // keys as k_klt_bin leaves them: sorted by (row, key column, index), with the first key of every row
    std::vector<uint64_t> K;
    for (int i = 0; i < NPTS; ++i)
        if (keyed(c[2 * i], c[2 * i + 1], W, H, bias)) K.push_back(splat_key((int)floor(c[2 * i + 1]) + bias, (int)floor(c[2 * i]) + bias, i));
    std::sort(K.begin(), K.end());
    std::vector<int> rs(H + 3, (int)K.size());
    for (int r = H + 1; r >= 0; --r) {
        rs[r] = rs[r + 1];
        while (rs[r] > 0 && key_y0(K[rs[r] - 1]) >= r) --rs[r];
    }
    std::vector<double> splat[NV];
    for (int v = 0; v < NV; ++v) splat[v].resize((size_t)H * W);
    for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) {
            int g[4][2];
            for (int h2 = 0; h2 < 2; ++h2) {
                const int kr = py - 1 + bias + h2, kx = px - 1 + bias;        // key row and column of y0 = py - 1 + h2, x0 = px - 1
                int q = kr < 0 ? 0 : rs[kr];
                const int hi = kr < 0 ? 0 : rs[kr + 1];
                if (bias) q = lower_x(K.data(), q, hi, kx);                   // the epiline model's search ...
                else while (q < hi && key_x0(K[q]) < kx) ++q;                 // ... and the KLT window's
                splat_runs(K.data(), q, hi, kx, g + 2 * h2);
            }
            double s[NV];
            splat_merge(K.data(), g, c.data(), V, s);
            for (int v = 0; v < NV; ++v) splat[v][py * W + px] = s[v];
        }
    double k0, k1;
    gauss3_sigma_half(k0, k1);
    int bad = 0;
    for (int v = 0; v < NV; ++v) {
        std::vector<double> val(NPTS);
        for (int i = 0; i < NPTS; ++i) val[i] = (double)planes[v][i];
        const std::vector<double> want = dense(H, W, c, val, k0, k1);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const double got = blur3_at(splat[v].data(), W, 0, 0, x, y, W, H, k0, k1, k0);
                if (std::memcmp(&got, &want[y * W + x], 8) != 0) {
                    std::printf("%d x %d bias %d NV %d plane %d pixel (%d, %d): %.17g, dense %.17g\n", H, W, bias, NV, v, y, x, got, want[y * W + x]);
                    ++bad;
                }
            }
    }
    return bad;
}

// the KLT's former hand-written reflect-101 against the border_map form that both trackers now share
int check_reflect() {
    int bad = 0;
    for (int len = 1; len <= 9; ++len)
        for (int p = -3 * len; p <= 3 * len; ++p) {
            int w = p;
            while (len > 1 && (w < 0 || w >= len)) w = w < 0 ? -w : 2 * len - 2 - w;
            if (len == 1) w = 0;
            if (reflect101(p, len) != w) { std::printf("reflect101(%d, %d) = %d, expected %d\n", p, len, reflect101(p, len), w); ++bad; }
        }
    return bad;
}

}  // namespace

int main() {
    Lcg rng = {20241018};
    int bad = check_reflect();
    const int frames[2][2] = {{5, 7}, {1, 4}};
    for (const auto& f : frames)
        for (int bias = 0; bias < 2; ++bias) {
            bad += check<1, double>(f[0], f[1], bias, rng);
            bad += check<2, float>(f[0], f[1], bias, rng);
        }
    std::printf("%d mismatches\n", bad);
    return bad ? 1 : 0;
}
