// Stand-alone host program of tests/test_cpu_mesh_cast.py::test_builder_under_address_and_ub_sanitizers: built together with
// nerfactor_amd/csrc/mesh_bvh.cpp as plain C++ with -fsanitize=address,undefined.  Each argument is a mesh file written by the
// test: int64 nv, int64 nf, float32 vertices [nv, 3], int32 faces [nf, 3].  Every mesh is built with max_leaf 1, 4 and nf into
// a buffer of exactly the queried size, twice, and the walk over the skip links must visit every triangle once.
#include <cstdio>
#include <cstring>
#include <vector>

#include "mesh_bvh.hpp"

using namespace nfx::mesh;

static int check(const std::vector<char>& blob, long long nf) {
    const Header* h = (const Header*)blob.data();
    char err[200];
    if (check_header(h, blob.size(), err, sizeof err)) return std::printf("header: %s\n", err), 1;
    const Node* nodes = (const Node*)(blob.data() + sizeof(Header));
    const Tri* tris = (const Tri*)(nodes + h->n_nodes + 1);
    std::vector<int> seen((size_t)nf, 0);
    long long covered = 0;
    for (int i = 0; i < h->n_nodes; ++i) {
        if (nodes[i].skip <= i || nodes[i].skip > h->n_nodes) return std::printf("skip link of node %d\n", i), 1;
        if (nodes[i].first < 0) continue;
        const int end = subtree_first(nodes[nodes[i].skip].first);
        for (int t = nodes[i].first; t < end; ++t, ++covered) {
            if (tris[t].orig < 0 || tris[t].orig >= nf || seen[(size_t)tris[t].orig]++) return std::printf("triangle %d\n", t), 1;
            const float* vs[3] = {tris[t].v0, tris[t].v1, tris[t].v2};
            for (const float* v : vs)
                for (int k = 0; k < 3; ++k)
                    if (!(nodes[i].lo[k] < v[k] && v[k] < nodes[i].hi[k])) return std::printf("box of node %d\n", i), 1;
        }
    }
    return covered == nf ? 0 : (std::printf("%lld of %lld triangles\n", covered, nf), 1);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        std::FILE* fh = std::fopen(argv[a], "rb");
        long long nv = 0, nf = 0;
        if (!fh || std::fread(&nv, 8, 1, fh) != 1 || std::fread(&nf, 8, 1, fh) != 1) return std::printf("cannot read %s\n", argv[a]), 1;
        std::vector<float> v((size_t)nv * 3);
        std::vector<int32_t> f((size_t)nf * 3);
        if (std::fread(v.data(), 4, v.size(), fh) != v.size() || std::fread(f.data(), 4, f.size(), fh) != f.size()) return 1;
        std::fclose(fh);
        const long long leafs[3] = {1, 4, nf};
        for (long long ml : leafs) {
            char err[200] = "";
            std::vector<char> b1(blob_bytes(nf, ml)), b2(b1.size());
            if (b1.empty() || build(v.data(), nv, f.data(), nf, (int)ml, b1.data(), b1.size(), err, sizeof err) ||
                build(v.data(), nv, f.data(), nf, (int)ml, b2.data(), b2.size(), err, sizeof err))
                return std::printf("%s max_leaf %lld: %s\n", argv[a], ml, err), 1;
            if (std::memcmp(b1.data(), b2.data(), b1.size())) return std::printf("two builds differ\n"), 1;
            if (check(b1, nf)) return 1;
            // the failures: a buffer one byte short, a face out of range, a non-finite vertex
            if (!build(v.data(), nv, f.data(), nf, (int)ml, b2.data(), b2.size() - 1, err, sizeof err)) return std::printf("short buffer accepted\n"), 1;
            std::vector<int32_t> fb(f);
            fb[fb.size() - 1] = (int32_t)nv;
            if (!build(v.data(), nv, fb.data(), nf, (int)ml, b2.data(), b2.size(), err, sizeof err)) return std::printf("bad face accepted\n"), 1;
            std::vector<float> vb(v);
            vb[0] = __builtin_nanf("");
            if (!build(vb.data(), nv, f.data(), nf, (int)ml, b2.data(), b2.size(), err, sizeof err)) return std::printf("NaN vertex accepted\n"), 1;
        }
        std::printf("%s: %lld triangles ok\n", argv[a], nf);
    }
    std::printf("MESH_BVH_SANITIZER_OK\n");
    return 0;
}
