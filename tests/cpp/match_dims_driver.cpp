// match_dims_driver.cpp -- pcc::matchRIFTFeaturesKnnBatch(pairs, dims) and pcc::matchRIFTFeaturesKnn(d1, d2, dims) on
// descriptor pairs read from a file (needs a GPU); tests/test_match_dims_gpu.py compares the printed rows with the Python
// binding's.
//   usage: match_dims_driver FILE DIMS
//   FILE: int32 n_pairs, then per pair int32 n1, int32 n2, n1 * 32 floats, n2 * 32 floats (native byte order)
//   prints per pair "B <p>: <row>" (the batch form) and "S <p>: <row>" (the single form), the row as the integers returned
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include "pcc/comparator_nn.hpp"

using namespace pcc;

static PointCloud<RIFT32>::Ptr read_cloud(std::ifstream& f, int32_t n) {
    PointCloud<RIFT32>::Ptr c(new PointCloud<RIFT32>);
    for (int32_t i = 0; i < n; ++i) {
        RIFT32 r;
        f.read(reinterpret_cast<char*>(r.histogram), sizeof(r.histogram));
        c->push_back(r);
    }
    return c;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::cerr << "usage: match_dims_driver FILE DIMS\n"; return 2; }
    const int dims = std::atoi(argv[2]);
    std::ifstream f(argv[1], std::ios::binary);
    int32_t n_pairs = 0;
    f.read(reinterpret_cast<char*>(&n_pairs), 4);
    std::vector<std::pair<PointCloud<RIFT32>::Ptr, PointCloud<RIFT32>::Ptr> > pairs;
    for (int32_t p = 0; p < n_pairs; ++p) {
        int32_t n[2];
        f.read(reinterpret_cast<char*>(n), 8);
        PointCloud<RIFT32>::Ptr a = read_cloud(f, n[0]);
        pairs.push_back(std::make_pair(a, read_cloud(f, n[1])));
    }
    if (!f) { std::cerr << "short file\n"; return 2; }
    try {
        const std::vector<std::vector<int> > batch = matchRIFTFeaturesKnnBatch(pairs, dims);
        for (size_t p = 0; p < pairs.size(); ++p) {
            std::cout << "B " << p << ":";
            for (int v : batch[p]) std::cout << " " << v;
            std::cout << "\n";
            const std::vector<int> single = matchRIFTFeaturesKnn(pairs[p].first, pairs[p].second, dims);
            std::cout << "S " << p << ":";
            for (int v : single) std::cout << " " << v;
            std::cout << "\n";
        }
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
