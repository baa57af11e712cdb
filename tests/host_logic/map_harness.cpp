// csrc/eds_map.hpp on the CPU: the serial forms of include/eds_hip_map.h's four clouds behind plain C entry points that
// tests/map_harness.py binds, and — with -DMAP_STANDALONE — a program of its own that runs a dumped set of cases (for a sanitizer build;
// it is never loaded into python that way).  Built with g++ -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../slam-eds_amd/csrc/eds_map.hpp"

using namespace edsmap;

extern "C" {

int map_sizes(int* fan, int* chunk) { *fan = FAN; *chunk = CHUNK; return (int)sizeof(Calib); }

// -1: the hosts decrease or leave 0 .. F - 1
int64_t map_window_cloud(int n, const int32_t* host, const float* uv, const float* ids, const float* calib, int F, uint32_t mask, const double* T_w_c,
                         int single_point, double* points, int32_t* per_host) {
    Runs r;
    if (!make_runs(n, host, F, &r)) return -1;
    selected_points(r, F, mask, per_host);
    const Calib c = {calib[0], calib[1], calib[2], calib[3]};
    return window_cloud(r, uv, ids, c, F, mask, T_w_c, single_point, points);
}

int map_window_depth_maps(int n, const int32_t* host, const float* uv, const float* ids, const float* calib, int F, uint32_t mask, const double* T_w_c,
                          int count, const double* T_dst_w, const double* K_dst, int dst_H, int dst_W, int64_t stride, double* xy, double* idp,
                          int32_t* src, int32_t* n_out) {
    Runs r;
    if (!make_runs(n, host, F, &r)) return -1;
    if (stride < selected_points(r, F, mask, nullptr)) return -1;
    const Calib c = {calib[0], calib[1], calib[2], calib[3]};
    window_depth_maps(r, uv, ids, c, F, mask, T_w_c, count, T_dst_w, K_dst, dst_H, dst_W, stride, xy, idp, src, n_out);
    return 0;
}

int64_t map_immature_cloud(int n_hosts, uint32_t mask, const int32_t* first, const float* uv, const float* idepth_min, const float* idepth_max,
                           const int32_t* status, const int32_t* alive, const double* T_w_c, const float* calib, int single_point, double* points,
                           double* colors, uint8_t* status_out) {
    const Calib c = {calib[0], calib[1], calib[2], calib[3]};
    return immature_cloud(n_hosts, mask, first, uv, idepth_min, idepth_max, status, alive, T_w_c, c, single_point, points, colors, status_out);
}

void map_slot_cloud(int n, const float* xn, const float* yn, const double* idp, const double* T_w_kf, double* points) {
    slot_cloud(n, xn, yn, idp, T_w_kf, points);
}

}  // extern "C"

#ifdef MAP_STANDALONE
// cases.bin: records of int32 {n, F, mask, count, dst_H, dst_W}, then host[n], uv[2n], ids[n], calib[4] (float), T_w_c[12 F], T_dst_w[12 count],
// K_dst[4 count] (double).  Every case runs both clouds and the depth maps into buffers of exactly the size they need.
template <class T> static bool take(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[6];
    int cases = 0;
    long long kept = 0;
    while (fread(hd, sizeof(int32_t), 6, f) == 6) {
        const int n = hd[0], F = hd[1], count = hd[3];
        std::vector<int32_t> host; std::vector<float> uv, ids, calib; std::vector<double> T, Td, K;
        if (!take(f, host, n) || !take(f, uv, 2 * (size_t)n) || !take(f, ids, n) || !take(f, calib, 4) || !take(f, T, 12 * (size_t)F) ||
            !take(f, Td, 12 * (size_t)count) || !take(f, K, 4 * (size_t)count)) return 3;
        int32_t per[8];
        Runs r;
        if (!make_runs(n, host.data(), F, &r)) return 4;
        const int nsel = selected_points(r, F, (uint32_t)hd[2], per);
        for (int single = 0; single < 2; ++single) {
            std::vector<double> pts((size_t)nsel * (single ? 1 : FAN) * 3);
            if (map_window_cloud(n, host.data(), uv.data(), ids.data(), calib.data(), F, (uint32_t)hd[2], T.data(), single, pts.data(), per) !=
                (int64_t)nsel * (single ? 1 : FAN)) return 5;
        }
        std::vector<double> xy((size_t)count * nsel * 2), idp((size_t)count * nsel);
        std::vector<int32_t> src((size_t)count * nsel), no(count);
        if (map_window_depth_maps(n, host.data(), uv.data(), ids.data(), calib.data(), F, (uint32_t)hd[2], T.data(), count, Td.data(), K.data(), hd[4],
                                  hd[5], nsel, xy.data(), idp.data(), src.data(), no.data())) return 6;
        for (int b = 0; b < count; ++b) kept += no[b];
        ++cases;
    }
    fclose(f);
    printf("%d cases, %lld points kept\n", cases, kept);
    return 0;
}
#endif
