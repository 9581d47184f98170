// example_text_map.cpp -- which pixels of a frame are text (STR_ER_WANT_TEXT_MAP) and which line each belongs to (STR_ER_WANT_LINE_MAP),
// written as PGM files; then the byte map of plane 0 (Y) again through ERFilter::text_map_regions, the single-stage form for ERs of a
// host plane, against the fused map restricted to that plane.
//
//   g++ -std=c++17 -O2 example_text_map.cpp -I../../include -L../lib -lstr_er_hip -o example_text_map
//   ./example_text_map strong.classifier weak.classifier frame.bgr width height out_dir
//
// frame.bgr is a raw interleaved 8-bit BGR dump.  Writes out_dir/text_map.pgm (255 where a strong or weak ER covers the pixel, 128
// where it is only a line member's, else 0 -- a redaction mask) and out_dir/line_map.pgm (the pixel's line id + 1, modulo 256).
// Prints "frame <width> <height> text <pixels> line <pixels> lines <n>", then whether the fused and the single-stage maps of
// plane 0 agree byte for byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "er_filter_hip.hpp"

using namespace str_er_host;

static bool write_pgm(const std::string &path, int w, int h, const std::vector<uint8_t> &pix)
{
    std::ofstream out(path, std::ios::binary);
    out << "P5\n" << w << " " << h << "\n255\n";
    out.write(reinterpret_cast<const char *>(pix.data()), (std::streamsize)pix.size());
    return (bool)out;
}

int main(int argc, char **argv)
{
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s strong.classifier weak.classifier frame.bgr width height out_dir\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
    if (w < 1 || h < 1) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> pix((size_t)w * h * 3);
    std::ifstream in(argv[3], std::ios::binary);
    if (!in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size())) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    const std::string dir = argv[6];
    try {
        ERFilter f(8, 120, 900000, 2, 0.7, 0.15, w, h, 1);
        f.set_stc(argv[1]);
        f.set_wtc(argv[2]);
        str_er_result *r = nullptr;
        int rc = str_er_detect_bgr(f.handle(), pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, 1, STR_ER_MEM_HOST,
                                   STR_ER_STAGE_ALL | STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_WANT_TEXT_MAP | STR_ER_WANT_LINE_MAP, &r);
        if (rc != STR_ER_OK) { std::fprintf(stderr, "detect: %s\n", str_er_last_error(f.handle())); return 1; }
        std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
        const std::vector<ERFilter::FrameMap> maps = ERFilter::frame_maps(r);
        if (maps.size() != 1 || maps[0].text.empty() || maps[0].line.empty()) { std::fprintf(stderr, "no maps\n"); return 1; }
        const ERFilter::FrameMap &m = maps[0];
        int32_t n_lines = 0;
        (void)str_er_result_texts(r, &n_lines);
        std::vector<uint8_t> redact(m.text.size()), lines(m.line.size());
        size_t n_text = 0, n_line = 0;
        for (size_t i = 0; i < m.text.size(); ++i) {
            const bool text = (m.text[i] & (STR_ER_TEXT_MAP_STRONG | STR_ER_TEXT_MAP_WEAK)) != 0, member = (m.text[i] & STR_ER_TEXT_MAP_LINE) != 0;
            redact[i] = text ? 255 : member ? 128 : 0;
            lines[i] = (uint8_t)((m.line[i] + 1) & 255);
            n_text += text;
            n_line += m.line[i] >= 0;
        }
        if (!write_pgm(dir + "/text_map.pgm", m.width, m.height, redact) || !write_pgm(dir + "/line_map.pgm", m.width, m.height, lines)) {
            std::fprintf(stderr, "cannot write to %s\n", dir.c_str());
            return 1;
        }
        std::printf("frame %d %d text %zu line %zu lines %d\n", m.width, m.height, n_text, n_line, n_lines);
        // plane 0 (Y) again, through the single-stage call on the plane compute_channels gives: its strong / weak ERs with their class
        // bits; against a call of the fused map that sees plane 0 only (str_er_detect_bgr_planes)
        std::vector<std::vector<uint8_t>> ch;
        f.compute_channels(Image8(pix.data(), w, h, 3 * (int64_t)w, 3), ch);
        int32_t n0 = 0;
        const str_er_cand *c0 = str_er_result_plane_cands(r, 0, &n0);
        std::vector<ER>      ers((size_t)n0);
        ERs                  list;
        std::vector<uint8_t> values;
        for (int32_t i = 0; i < n0; ++i) {
            if (c0[i].cls == STR_ER_CLS_POOL) continue;
            ER &e = ers[(size_t)i];
            e.bound.x = c0[i].x; e.bound.y = c0[i].y; e.bound.width = c0[i].w; e.bound.height = c0[i].h;
            e.level = c0[i].level; e.key = c0[i].key; e.area = (int)c0[i].area;
            list.push_back(&e);
            values.push_back(c0[i].cls == STR_ER_CLS_STRONG ? STR_ER_TEXT_MAP_STRONG : STR_ER_TEXT_MAP_WEAK);
        }
        const ERFilter::FrameMap single = f.text_map_regions(Image8(ch[0].data(), w, h, w, 1), list, values, w, h);
        const int32_t        n_sel = str_er_result_n_planes(r);         // (one level: a flag per channel)
        std::vector<uint8_t> sel((size_t)n_sel, 0);
        sel[0] = 1;
        str_er_result *r0 = nullptr;
        rc = str_er_detect_bgr_planes(f.handle(), pix.data(), w, h, 3 * (int64_t)w, 3 * (int64_t)w * h, 1, STR_ER_MEM_HOST,
                                      STR_ER_STAGE_ALL | STR_ER_WANT_TEXT_MAP, sel.data(), n_sel, &r0);
        if (rc != STR_ER_OK) { std::fprintf(stderr, "detect (plane 0): %s\n", str_er_last_error(f.handle())); return 1; }
        std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard0(r0, str_er_result_free);
        const std::vector<ERFilter::FrameMap> fused0 = ERFilter::frame_maps(r0);
        const bool same = fused0.size() == 1 && fused0[0].text == single.text;
        std::printf("plane 0: %zu ERs, fused == single-stage: %s\n", list.size(), same ? "yes" : "no");
        return same ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
