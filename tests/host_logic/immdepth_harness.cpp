// csrc/eds_immdepth.hpp on the CPU: the entry points tests/immdepth_harness.py binds, and — with -DIMD_STANDALONE — a program of its own
// that runs a dumped set of cases plus degenerate inputs (for a sanitizer build; it is never loaded into python that way).
// Built with g++ -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../slam-eds_amd/csrc/eds_immdepth.hpp"
#include "../../slam-eds_amd/csrc/eds_kdbuild.hpp"

using edsimm::Params;
using edsimm::Point;

static_assert(sizeof(Point) == 128, "the python side reads a point as 32 words");

extern "C" {

int imd_point_size(void) { return (int)sizeof(Point); }
int imd_capacity(void) { return edskdb::CAPACITY; }
void imd_build_tree(const double* xy, int m, int* perm) { edskd::build_tree(xy, m, perm); }
// 1: the device build's rule says unambiguous and finite, so the device builds the tree
int imd_build_sorted(const double* xy, int m, int* perm) { return edskdb::build_sorted(xy, m, perm) ? 1 : 0; }
int imd_map_finite(const double* xy, int m) { return edsimd::map_finite(xy, m) ? 1 : 0; }

// steps 1 to 4 for n pixels
void imd_nearest(const double* txy, const double* tidp, const int32_t* perm, int m, int n, const int32_t* uv, double sx, double sy, int32_t* pos,
                 int32_t* index, float* idepth, double* distance) {
    for (int i = 0; i < n; ++i) {
        const edsimd::Nearest r = edsimd::nearest(txy, tidp, perm, m, uv[2 * i], uv[2 * i + 1], sx, sy);
        pos[i] = r.pos; index[i] = r.index; idepth[i] = r.idepth; distance[i] = r.distance;
    }
}

// the whole loop
void imd_seed(const float* c, int H, int W, const Params* s, const double* txy, const double* tidp, const int32_t* perm, int m, int n,
              const int32_t* uv, const float* type, double sx, double sy, Point* out, int32_t* index, float* idepth, double* distance) {
    for (int i = 0; i < n; ++i) {
        const edsimd::Nearest r = edsimd::seed(out[i], c, W, H, *s, uv[2 * i], uv[2 * i + 1], type[i], txy, tidp, perm, m, sx, sy);
        index[i] = r.index; idepth[i] = r.idepth; distance[i] = r.distance;
    }
}

// the loop composed by hand from edskd::nn and edsimm::construct, without edsimd::
void imd_composed(const float* c, int H, int W, const Params* s, const double* txy, const double* tidp, const int32_t* perm, int m, int n,
                  const int32_t* uv, const float* type, double sx, double sy, Point* out, int32_t* index, float* idepth, double* distance) {
    for (int i = 0; i < n; ++i) {
        const int u = uv[2 * i], v = uv[2 * i + 1];
        if (m < 1) {
            edsimm::construct(out[i], c, W, H, *s, u, v, type[i], false, 0.0f, 0.0);
            index[i] = -1; idepth[i] = 0.0f; distance[i] = 0.0;
            continue;
        }
        const volatile double qx = (double)u * sx, qy = (double)v * sy;
        const int k = edskd::nn(txy, m, qx, qy, nullptr);
        const volatile double dx = txy[2 * k] - (double)u, dy = txy[2 * k + 1] - (double)v;
        const volatile double xx = dx * dx, yy = dy * dy;
        const double dist = sqrt(xx + yy);
        const float idp = (float)tidp[k];
        edsimm::construct(out[i], c, W, H, *s, u, v, type[i], true, idp, dist);
        index[i] = perm[k]; idepth[i] = idp; distance[i] = dist;
    }
}

}  // extern "C"

#ifdef IMD_STANDALONE
namespace {

template <class T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

bool same(const void* a, const void* b, size_t bytes) { return bytes == 0 || memcmp(a, b, bytes) == 0; }

int run_case(int H, int W, const Params& prm, const std::vector<float>& img, int m, const std::vector<double>& xy, const std::vector<double>& idp, int n,
             const std::vector<int32_t>& uv, const std::vector<float>& type, double sx, double sy) {
    std::vector<int> perm((size_t)m + 1);
    std::vector<double> txy(2 * (size_t)m + 2), tidp((size_t)m + 1);
    if (m > 0) edskd::build_tree(xy.data(), m, perm.data());
    for (int p = 0; p < m; ++p) { txy[2 * p] = xy[2 * perm[p]]; txy[2 * p + 1] = xy[2 * perm[p] + 1]; tidp[p] = idp[perm[p]]; }
    std::vector<Point> a((size_t)n + 1), b((size_t)n + 1);
    std::vector<int32_t> ia((size_t)n + 1), ib((size_t)n + 1), pos((size_t)n + 1), ic((size_t)n + 1);
    std::vector<float> da((size_t)n + 1), db((size_t)n + 1), dc((size_t)n + 1);
    std::vector<double> ra((size_t)n + 1), rb((size_t)n + 1), rc((size_t)n + 1);
    imd_seed(img.data(), H, W, &prm, txy.data(), tidp.data(), perm.data(), m, n, uv.data(), type.data(), sx, sy, a.data(), ia.data(), da.data(), ra.data());
    imd_composed(img.data(), H, W, &prm, txy.data(), tidp.data(), perm.data(), m, n, uv.data(), type.data(), sx, sy, b.data(), ib.data(), db.data(), rb.data());
    int bad = 0;
    if (!same(a.data(), b.data(), (size_t)n * sizeof(Point)) || !same(ia.data(), ib.data(), (size_t)n * 4) || !same(da.data(), db.data(), (size_t)n * 4) ||
        !same(ra.data(), rb.data(), (size_t)n * 8)) ++bad;
    imd_nearest(txy.data(), tidp.data(), perm.data(), m, n, uv.data(), sx, sy, pos.data(), ic.data(), dc.data(), rc.data());
    if (!same(ia.data(), ic.data(), (size_t)n * 4) || !same(da.data(), dc.data(), (size_t)n * 4) || !same(ra.data(), rc.data(), (size_t)n * 8)) ++bad;
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t ncases = 0;
    if (!rd(f, &ncases, 1)) return 2;
    int bad = 0, pixels = 0;
    Params prm;
    for (int c = 0; c < ncases; ++c) {
        int32_t hd[4];
        double sc[2];
        if (!rd(f, hd, 4) || !rd(f, sc, 2) || !rd(f, &prm, 1)) return 2;
        const int H = hd[0], W = hd[1], m = hd[2], n = hd[3];
        std::vector<float> img((size_t)H * W), type((size_t)n);
        std::vector<double> xy(2 * (size_t)m), idp((size_t)m);
        std::vector<int32_t> uv(2 * (size_t)n);
        if (!rd(f, img.data(), img.size()) || !rd(f, xy.data(), xy.size()) || !rd(f, idp.data(), idp.size()) || !rd(f, uv.data(), uv.size()) ||
            !rd(f, type.data(), type.size())) return 2;
        bad += run_case(H, W, prm, img, m, xy, idp, n, uv, type, sc[0], sc[1]);
        pixels += n;
    }
    fclose(f);
    // degenerate inputs of its own: no pixels, no map, one point, pixels far outside the image, extreme scales
    {
        const int H = 16, W = 16;
        std::vector<float> img((size_t)H * W, 10.0f);
        const Params p0 = edsimm::params_default();
        std::vector<double> xy = {3.5, 4.25}, idp = {0.5};
        std::vector<int32_t> uv = {8, 8, -2147483647 - 1, 2147483647, 0, 0, 15, 15, 1 << 30, -(1 << 30)};
        std::vector<float> type = {1, 2, 4, 1, 2};
        bad += run_case(H, W, p0, img, 0, {}, {}, 0, {}, {}, 1.0, 1.0);
        bad += run_case(H, W, p0, img, 0, {}, {}, 5, uv, type, 1.0, 1.0);
        bad += run_case(H, W, p0, img, 1, xy, idp, 5, uv, type, 1.0, 1.0);
        bad += run_case(H, W, p0, img, 1, xy, idp, 5, uv, type, 1e300, -1e300);
        bad += run_case(H, W, p0, img, 1, xy, idp, 5, uv, type, 0.0, 0.0);
    }
    printf("%d cases, %d pixels, %d mismatches\n", (int)ncases, pixels, bad);
    return bad ? 1 : 0;
}
#endif
