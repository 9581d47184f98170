// Host-only check of csrc/stage_rules.h (compiled and run by tests/test_host_cpp.py): check_stages against the flag checks as every detect entry
// point made them one by one before they were gathered there -- transcribed below in their order, with their messages -- for every combination
// of the 17 flag bits, every call shape and both states of the context.  The code must agree everywhere, and so must the first STR_ER_* name of
// the message (the message may be worded otherwise).
#include <stdio.h>
#include <string.h>

#include <string>

#include "stage_rules.h"

using namespace str_er_host;

namespace {

struct Ref { int code; std::string msg; };
struct Ctx { bool cascades, svm1800; };
#define FAIL(code, msg) return Ref{code, msg}

// run_batch's checks, in their order (ppi: planes_per_image; frames: !frame_wh.empty())
Ref ref_run_batch(uint32_t stages, const Ctx &c, int ppi, bool frames)
{
    if ((stages & STR_ER_STAGE_CLASSIFY) && !c.cascades) FAIL(STR_ER_ESTATE, "classify needs both cascades (str_er_load_cascade)");
    if (!(stages & STR_ER_STAGE_EXTRACT)) FAIL(STR_ER_EINVAL, "stages must include STR_ER_STAGE_EXTRACT");
    if ((stages & STR_ER_STAGE_CLASSIFY) && !(stages & STR_ER_STAGE_NMS)) FAIL(STR_ER_EINVAL, "STR_ER_STAGE_CLASSIFY needs STR_ER_STAGE_NMS");
    if ((stages & STR_ER_STAGE_OCR) && !(stages & STR_ER_STAGE_CLASSIFY)) FAIL(STR_ER_EINVAL, "STR_ER_STAGE_OCR needs STR_ER_STAGE_CLASSIFY");
    if ((stages & STR_ER_STAGE_OCR) && !c.svm1800) FAIL(STR_ER_ESTATE, "STR_ER_STAGE_OCR needs an SVM model loaded with dim = 1800 (str_er_load_svm_model)");
    if ((stages & STR_ER_STAGE_TRACK) && !(stages & STR_ER_STAGE_CLASSIFY)) FAIL(STR_ER_EINVAL, "STR_ER_STAGE_TRACK needs STR_ER_STAGE_CLASSIFY");
    if ((stages & (STR_ER_STAGE_GROUP | STR_ER_GROUP_INNER_SUP | STR_ER_GROUP_OVERLAP_SUP)) && !(stages & STR_ER_STAGE_TRACK)) FAIL(STR_ER_EINVAL, "STR_ER_STAGE_GROUP needs STR_ER_STAGE_TRACK");
    if ((stages & (STR_ER_GROUP_INNER_SUP | STR_ER_GROUP_OVERLAP_SUP)) && !(stages & STR_ER_STAGE_GROUP)) FAIL(STR_ER_EINVAL, "STR_ER_GROUP_INNER_SUP / _OVERLAP_SUP modify STR_ER_STAGE_GROUP");
    if ((stages & STR_ER_STAGE_OCR_LINES) && !(stages & STR_ER_STAGE_GROUP)) FAIL(STR_ER_EINVAL, "STR_ER_STAGE_OCR_LINES needs STR_ER_STAGE_GROUP");
    if ((stages & (STR_ER_WANT_LINE_CROPS | STR_ER_WANT_LINE_GLYPHS)) && !(stages & STR_ER_STAGE_GROUP))
        FAIL(STR_ER_EINVAL, "STR_ER_WANT_LINE_CROPS / _GLYPHS need STR_ER_STAGE_GROUP");
    if ((stages & STR_ER_WANT_LINE_GLYPHS) && !(stages & STR_ER_WANT_LINE_CROPS)) FAIL(STR_ER_EINVAL, "STR_ER_WANT_LINE_GLYPHS needs STR_ER_WANT_LINE_CROPS");
    if ((stages & STR_ER_WANT_TEXT_MAP) && !(stages & STR_ER_STAGE_CLASSIFY)) FAIL(STR_ER_EINVAL, "STR_ER_WANT_TEXT_MAP needs STR_ER_STAGE_CLASSIFY");
    if ((stages & STR_ER_WANT_LINE_MAP) && !(stages & STR_ER_STAGE_GROUP)) FAIL(STR_ER_EINVAL, "STR_ER_WANT_LINE_MAP needs STR_ER_STAGE_GROUP");
    if ((stages & (STR_ER_WANT_TEXT_MAP | STR_ER_WANT_LINE_MAP)) && !frames)
        FAIL(STR_ER_EINVAL, "STR_ER_WANT_TEXT_MAP / _LINE_MAP need frames (not the per-plane calls or the strip path)");
    if ((stages & STR_ER_STAGE_OCR_LINES) && !c.svm1800)
        FAIL(STR_ER_ESTATE, "STR_ER_STAGE_OCR_LINES needs an SVM model loaded with dim = 1800 (str_er_load_svm_model)");
    if ((stages & STR_ER_STAGE_TRACK) && ppi <= 0) FAIL(STR_ER_EINVAL, "STR_ER_STAGE_TRACK needs BGR frames (calc_color reads the YCrCb image)");
    return Ref{STR_ER_OK, ""};
}

// text_map_reserve's checks (the uniform and list frame calls, before they stage anything)
Ref ref_text_map_reserve(uint32_t stages)
{
    const bool map = (stages & STR_ER_WANT_TEXT_MAP) != 0, ids = (stages & STR_ER_WANT_LINE_MAP) != 0;
    if (!map && !ids) return Ref{STR_ER_OK, ""};
    if (map && !(stages & STR_ER_STAGE_CLASSIFY)) FAIL(STR_ER_EINVAL, "STR_ER_WANT_TEXT_MAP needs STR_ER_STAGE_CLASSIFY");
    if (ids && !(stages & STR_ER_STAGE_GROUP)) FAIL(STR_ER_EINVAL, "STR_ER_WANT_LINE_MAP needs STR_ER_STAGE_GROUP");
    return Ref{STR_ER_OK, ""};
}

// str_er_detect_bgr / _nv12 / _bgr_list / _nv12_list: text_map_reserve, then run_batch with every plane of the frames
Ref ref_frames(uint32_t stages, const Ctx &c)
{
    const Ref r = ref_text_map_reserve(stages);
    if (r.code != STR_ER_OK) return r;
    return ref_run_batch(stages, c, 3, true);
}

// str_er_detect_bgr_planes: the subset's check, then detect_bgr_impl (text_map_reserve, run_batch with planes_per_image = 0)
Ref ref_bgr_planes(uint32_t stages, const Ctx &c)
{
    if (stages & (STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_STAGE_OCR_LINES))
        FAIL(STR_ER_EINVAL, "er_track / er_grouping read every plane of an image: not with a plane subset");
    const Ref r = ref_text_map_reserve(stages);
    if (r.code != STR_ER_OK) return r;
    return ref_run_batch(stages, c, 0, true);
}

// str_er_detect_planes / _planes_list: no maps, then run_batch without frames
Ref ref_planes(uint32_t stages, const Ctx &c)
{
    if (stages & (STR_ER_WANT_TEXT_MAP | STR_ER_WANT_LINE_MAP))
        FAIL(STR_ER_EINVAL, "STR_ER_WANT_TEXT_MAP / _LINE_MAP need frames: not with str_er_detect_planes");
    return ref_run_batch(stages, c, 0, false);
}

// str_er_strip_merge_ex: what the strip path does not make, then run_batch without frames (planes_per_image > 0 when every plane is merged)
Ref ref_strip(uint32_t stages, const Ctx &c, bool all_planes)
{
    if (stages & STR_ER_WANT_MASKS) FAIL(STR_ER_EINVAL, "STR_ER_WANT_MASKS is not supported by the strip path (str_er_strip_merge)");
    if (stages & STR_ER_WANT_SHAPES) FAIL(STR_ER_EINVAL, "STR_ER_WANT_SHAPES is not supported by the strip path (str_er_strip_merge)");
    if (stages & STR_ER_WANT_STROKES) FAIL(STR_ER_EINVAL, "STR_ER_WANT_STROKES is not supported by the strip path (str_er_strip_merge)");
    if (stages & (STR_ER_WANT_TEXT_MAP | STR_ER_WANT_LINE_MAP))
        FAIL(STR_ER_EINVAL, "STR_ER_WANT_TEXT_MAP / _LINE_MAP are not supported by the strip path (str_er_strip_merge)");
    if (stages & (STR_ER_WANT_LINE_CROPS | STR_ER_WANT_LINE_GLYPHS))
        FAIL(STR_ER_EINVAL, "STR_ER_WANT_LINE_CROPS / _GLYPHS are not supported by the strip path (str_er_strip_merge)");
    return ref_run_batch(stages, c, all_planes ? 3 : 0, false);
}

// the first STR_ER_ name of a message ("" when it has none)
std::string first_name(const char *m)
{
    if (!m) return "";
    const char *p = strstr(m, "STR_ER_");
    if (!p) return "";
    size_t n = 0;
    while (p[n] == '_' || (p[n] >= 'A' && p[n] <= 'Z') || (p[n] >= '0' && p[n] <= '9')) ++n;
    return std::string(p, n);
}

} // namespace

int main()
{
    struct Shape { const char *name; CallShape k; int ref; };
    const Shape shapes[] = {
        {"frames", {true, true, false, false}, 0},
        {"bgr_planes", {true, false, false, true}, 1},
        {"planes", {false, false, false, false}, 2},
        {"strip (every plane)", {false, true, true, false}, 3},
        {"strip (a subset)", {false, false, true, false}, 4},
    };
    long checked = 0, rejected = 0, bad = 0;
    for (const Shape &s : shapes)
        for (int cs = 0; cs < 4; ++cs) {
            const Ctx c{(cs & 1) != 0, (cs & 2) != 0};
            for (uint32_t st = 0; st < (1u << 17); ++st) {
                const Ref want = s.ref == 0 ? ref_frames(st, c) : s.ref == 1 ? ref_bgr_planes(st, c) : s.ref == 2 ? ref_planes(st, c)
                                                                            : ref_strip(st, c, s.ref == 3);
                const StageVerdict got = check_stages(st, s.k, c.cascades, c.svm1800);
                ++checked;
                rejected += want.code != STR_ER_OK;
                const std::string wn = want.code == STR_ER_OK ? "" : first_name(want.msg.c_str()), gn = first_name(got.msg);
                if (got.code != want.code || gn != wn || (got.code != STR_ER_OK) != (got.msg != nullptr)) {
                    if (++bad <= 10)
                        printf("MISMATCH %s cascades %d svm %d stages 0x%05x: want %d '%s', got %d '%s'\n", s.name, (int)c.cascades, (int)c.svm1800, st,
                               want.code, want.msg.c_str(), got.code, got.msg ? got.msg : "");
                }
            }
        }
    if (bad) { printf("stage rules: %ld of %ld combinations differ\n", bad, checked); return 1; }
    printf("stage rules ok: %ld combinations (%ld rejected)\n", checked, rejected);
    return 0;
}
