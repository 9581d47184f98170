// example_image_batch.cpp -- the reference's image mode over several photographs of different sizes in ONE call
// (ERFilter::text_detect_batch -> str_er_detect_bgr_list), checked against one text_detect call per photograph.
//
//   g++ -std=c++17 -O2 example_image_batch.cpp -I../../include -L../lib -lstr_er_hip -o example_image_batch
//   ./example_image_batch strong.classifier weak.classifier a.bgr 640 480 b.bgr 320 240 ...
//
// Each .bgr is a raw interleaved 8-bit BGR dump.  Prints one line per frame and plane, then whether the batch agrees with the
// single-frame calls (same planes, nodes, pools, strong / weak ERs and scores).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "er_filter_hip.hpp"

using namespace str_er_host;

static bool same_ers(const ERs &a, const ERs &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i]->key != b[i]->key || a[i]->area != b[i]->area || a[i]->level != b[i]->level || a[i]->score_strong != b[i]->score_strong ||
            a[i]->score_weak != b[i]->score_weak)
            return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 6 || (argc - 3) % 3 != 0) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier frame.bgr width height [frame.bgr width height ...]\n", argv[0]);
        return 2;
    }
    const int nf = (argc - 3) / 3;
    std::vector<std::vector<uint8_t>> pix((size_t)nf);
    std::vector<Image8> frames;
    int max_w = 1, max_h = 1;
    for (int f = 0; f < nf; ++f) {
        const int w = std::atoi(argv[4 + 3 * f]), h = std::atoi(argv[5 + 3 * f]);
        pix[(size_t)f].resize((size_t)w * h * 3);
        std::ifstream in(argv[3 + 3 * f], std::ios::binary);
        if (!in.read(reinterpret_cast<char *>(pix[(size_t)f].data()), (std::streamsize)pix[(size_t)f].size())) { std::fprintf(stderr, "short read\n"); return 2; }
        frames.emplace_back(pix[(size_t)f].data(), w, h, (int64_t)w * 3, 3);
        max_w = std::max(max_w, w); max_h = std::max(max_h, h);
    }
    try {
        ERFilter er_filter(8, 120, 900000, 2, 0.7, 0.15, max_w, max_h, nf);
        er_filter.set_stc(argv[1]);
        er_filter.set_wtc(argv[2]);
        std::vector<std::vector<ERTree>> trees;
        std::vector<ERs> root;
        std::vector<std::vector<ERs>> pool, strong, weak;
        er_filter.text_detect_batch(frames, trees, root, pool, strong, weak);
        bool same = (int)trees.size() == nf;
        for (int f = 0; same && f < nf; ++f) {
            std::vector<ERTree> t1;
            ERs r1;
            std::vector<ERs> a1, p1, s1, w1;
            er_filter.text_detect(frames[(size_t)f], t1, r1, a1, p1, s1, w1);
            same = t1.size() == trees[(size_t)f].size();
            for (size_t i = 0; same && i < t1.size(); ++i) {
                std::printf("frame %d plane %zu kept %zu pool %zu strong %zu weak %zu\n", f, i, trees[(size_t)f][i].nodes.size(), pool[(size_t)f][i].size(),
                            strong[(size_t)f][i].size(), weak[(size_t)f][i].size());
                same = t1[i].nodes.size() == trees[(size_t)f][i].nodes.size() && same_ers(p1[i], pool[(size_t)f][i]) && same_ers(s1[i], strong[(size_t)f][i]) &&
                       same_ers(w1[i], weak[(size_t)f][i]) && r1[i]->area == root[(size_t)f][i]->area;
                for (size_t k = 0; same && k < t1[i].nodes.size(); ++k)
                    same = t1[i].nodes[k].key == trees[(size_t)f][i].nodes[k].key && t1[i].nodes[k].area == trees[(size_t)f][i].nodes[k].area;
            }
        }
        std::printf("batch == per frame: %s\n", same ? "yes" : "NO");
        return same ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
}
