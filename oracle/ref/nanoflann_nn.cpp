// Replays the reference's own nanoflann (src/utils/nanoflann.h, included unmodified) on a case file the way CoarseInitializer::makeNN
// (CoarseInitializer.cpp:888-946) calls it: a 2-D fp32 index with leaf size 5 per level, ten neighbours of every point in its own level
// and the one nearest point of the level above to 0.5f pt - 0.25f.  Test infrastructure: oracle/ref/Makefile builds it into
// oracle/_ref/nanoflann_nn with the reference's flags; oracle/ref/refcase.py writes the case and reads the answer.
//   case file : int32 n, float32 uv[n][2], int32 n_up, float32 uv_up[n_up][2]
//   answer    : int32 nb[n][10], float32 dist[n][10], int32 parent[n], float32 parent_dist[n]
// ret_index holds -1 and ret_dist 0 before every init(): with fewer than ten points nanoflann leaves the tail unwritten (and init()
// itself writes FLT_MAX into the last distance).  n_up = 0: parent -1, parent_dist 0.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "nanoflann.h"

// the data set as nanoflann's interface asks for it (the four members of its DatasetAdaptor): packed fp32 (u, v)
struct Cloud {
    const float* uv;
    size_t n;
    inline size_t kdtree_get_point_count() const { return n; }
    inline float kdtree_distance(const float* q, const size_t j, size_t /*dim*/) const {
        const float d0 = q[0] - uv[2 * j];
        const float d1 = q[1] - uv[2 * j + 1];
        return d0 * d0 + d1 * d1;
    }
    inline float kdtree_get_pt(const size_t j, int dim) const { return uv[2 * j + (dim == 0 ? 0 : 1)]; }
    template <class BBOX> bool kdtree_get_bbox(BBOX&) const { return false; }
};

typedef nanoflann::KDTreeSingleIndexAdaptor<nanoflann::L2_Simple_Adaptor<float, Cloud>, Cloud, 2> Tree;

static bool read_points(FILE* f, std::vector<float>& v) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0) return false;
    v.assign(2 * (size_t)n, 0.0f);
    return !n || fread(v.data(), 4, v.size(), f) == v.size();
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: nanoflann_nn case.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    std::vector<float> uv, up;
    if (!f || !read_points(f, uv) || !read_points(f, up)) { fprintf(stderr, "bad case file\n"); return 1; }
    fclose(f);
    const int nn = 10;
    const size_t n = uv.size() / 2, n_up = up.size() / 2;
    Cloud pc{uv.data(), n}, pc_up{up.data(), n_up};
    Tree index(2, pc, nanoflann::KDTreeSingleIndexAdaptorParams(5)), index_up(2, pc_up, nanoflann::KDTreeSingleIndexAdaptorParams(5));
    index.buildIndex();
    index_up.buildIndex();
    std::vector<int32_t> nb(n * nn), parent(n);
    std::vector<float> dist(n * nn), parent_dist(n);
    int ret_index[nn];
    float ret_dist[nn];
    nanoflann::KNNResultSet<float, int, int> resultSet(nn);
    nanoflann::KNNResultSet<float, int, int> resultSet1(1);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < nn; ++k) { ret_index[k] = -1; ret_dist[k] = 0.0f; }
        resultSet.init(ret_index, ret_dist);
        float pt[2] = {uv[2 * i], uv[2 * i + 1]};
        index.findNeighbors(resultSet, pt, nanoflann::SearchParams());
        for (int k = 0; k < nn; ++k) { nb[i * nn + k] = ret_index[k]; dist[i * nn + k] = ret_index[k] < 0 ? 0.0f : ret_dist[k]; }
        parent[i] = -1;
        parent_dist[i] = 0.0f;
        if (n_up) {
            ret_index[0] = -1;
            resultSet1.init(ret_index, ret_dist);
            pt[0] = pt[0] * 0.5f - 0.25f;
            pt[1] = pt[1] * 0.5f - 0.25f;
            index_up.findNeighbors(resultSet1, pt, nanoflann::SearchParams());
            parent[i] = ret_index[0];
            parent_dist[i] = ret_index[0] < 0 ? 0.0f : ret_dist[0];
        }
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    fwrite(nb.data(), 4, nb.size(), o);
    fwrite(dist.data(), 4, dist.size(), o);
    fwrite(parent.data(), 4, parent.size(), o);
    fwrite(parent_dist.data(), 4, parent_dist.size(), o);
    return fclose(o) == 0 ? 0 : 1;
}
