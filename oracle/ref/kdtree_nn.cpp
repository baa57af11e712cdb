// Replays the reference's own k-d tree (src/utils/KDTree.hpp, included unmodified) on a case file: the nearest depth-map point of
// every query, as KeyFrame::setDepthMap (KeyFrame.cpp:1151-1158) asks for it.  Test infrastructure: oracle/ref/Makefile builds it
// into oracle/_ref/kdtree_nn with the reference's flags; oracle/ref/refcase.py writes the case and reads the answer.
//   case file : int32 m, float64 depth_xy[m][2], int32 n, float64 query_xy[n][2]
//   answer    : int32 idx[n] (nnSearch), float64 min_dist[n] (its minDist)
#include <array>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "KDTree.hpp"

// the 2-D point the tree is instantiated with: eds::mapping::Point<double> (src/mapping/Types.hpp:39-71) — an std::array<T, 2>
// with DIM = 2
struct Point2 : public std::array<double, 2> {
    static const int DIM = 2;
    Point2() : std::array<double, 2>{{0.0, 0.0}} {}
    Point2(double x, double y) : std::array<double, 2>{{x, y}} {}
};

static bool read_points(FILE* f, std::vector<Point2>& v) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0) return false;
    std::vector<double> xy(2 * (size_t)n);
    if (n && fread(xy.data(), 8, xy.size(), f) != xy.size()) return false;
    v.clear();
    for (int32_t i = 0; i < n; ++i) v.emplace_back(xy[2 * i], xy[2 * i + 1]);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: kdtree_nn case.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    std::vector<Point2> depth, query;
    if (!f || !read_points(f, depth) || !read_points(f, query) || depth.empty()) { fprintf(stderr, "bad case file\n"); return 1; }
    fclose(f);
    eds::mapping::KDTree<Point2> kdtree(depth);
    std::vector<int32_t> idx(query.size());
    std::vector<double> dist(query.size());
    for (size_t i = 0; i < query.size(); ++i) idx[i] = kdtree.nnSearch(query[i], &dist[i]);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    fwrite(idx.data(), 4, idx.size(), o);
    fwrite(dist.data(), 8, dist.size(), o);
    return fclose(o) == 0 ? 0 : 1;
}
