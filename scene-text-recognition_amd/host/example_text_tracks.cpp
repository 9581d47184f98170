// example_text_tracks.cpp -- text tracks over a short video: the lines of consecutive frames that are the same text share an id
// (STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS), within a call and, with ERFilter::TextTracker, across calls.
//
//   g++ -std=c++17 -O2 example_text_tracks.cpp -I../../include -L../lib -lstr_er_hip -o example_text_tracks
//   ./example_text_tracks strong.classifier weak.classifier video.bgr width height frames [frames per call = 4] [pyramid levels = 3]
//
// video.bgr holds `frames` raw interleaved 8-bit BGR frames back to back.  Prints one row per frame: "frame <n>:" and, per frame
// line of the frame, "<id>@<x>,<y>,<w>x<h>" with the persistent id of its representative and the frame line's box.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <vector>

#include "er_filter_hip.hpp"

using namespace str_er_host;

int main(int argc, char **argv)
{
    if (argc < 7 || argc > 9) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier video.bgr width height frames [frames per call] [pyramid levels]\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[4]), h = std::atoi(argv[5]), frames = std::atoi(argv[6]);
    const int per_call = argc > 7 ? std::atoi(argv[7]) : 4, levels = argc > 8 ? std::atoi(argv[8]) : 3;
    if (w < 1 || h < 1 || frames < 1 || per_call < 1 || levels < 1) { std::fprintf(stderr, "bad arguments\n"); return 2; }
    const size_t frame_bytes = (size_t)w * h * 3;
    std::vector<uint8_t> pix(frame_bytes * (size_t)frames);
    std::ifstream in(argv[3], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size())) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    str_er_params p;
    str_er_default_params(&p);
    p.max_width = w; p.max_height = h; p.max_frames = per_call; p.n_pyr_levels = levels;
    str_er_ctx *c = nullptr;
    if (str_er_create(&p, &c) != STR_ER_OK) { std::fprintf(stderr, "create: %s\n", str_er_last_error(nullptr)); return 1; }
    std::unique_ptr<str_er_ctx, void (*)(str_er_ctx *)> ctx(c, str_er_destroy);
    if (str_er_load_cascade(c, 0, argv[1]) != STR_ER_OK || str_er_load_cascade(c, 1, argv[2]) != STR_ER_OK) {
        std::fprintf(stderr, "cascades: %s\n", str_er_last_error(c));
        return 1;
    }
    ERFilter::TextTracker tracker;
    for (int f0 = 0; f0 < frames; f0 += per_call) {
        const int n = std::min(per_call, frames - f0);
        str_er_result *r = nullptr;
        const int rc = str_er_detect_bgr(c, pix.data() + frame_bytes * (size_t)f0, w, h, 3 * (int64_t)w, (int64_t)frame_bytes, n, STR_ER_MEM_HOST,
                                         STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_FRAME_LINES | STR_ER_WANT_LINE_LINKS, &r);
        if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(c)); return 1; }
        std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
        const ERFilter::FrameLines fl = ERFilter::frame_lines(r);
        std::vector<int64_t> ids;
        try {
            ids = tracker.update(c, ERFilter::line_links(r));
        } catch (const std::exception &e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 1;
        }
        size_t at = 0;
        for (int k = 0; k < n; ++k) {
            std::printf("frame %d:", f0 + k);
            for (; at < fl.lines.size() && fl.lines[at].frame == (uint32_t)k; ++at) {
                const str_er_frame_line &g = fl.lines[at];
                std::printf(" %lld@%d,%d,%dx%d", (long long)ids[(size_t)g.rep], g.x, g.y, g.w, g.h);
            }
            std::printf("\n");
        }
    }
    return 0;
}
