// stage_rules.h -- INTERNAL: which STR_ER_STAGE_* / STR_ER_WANT_* combinations a detect call accepts, in one place.  HIP-free: every detect entry point
// asks it after its argument checks and before it stages, uploads, allocates or enqueues anything (tests/cpp/stage_rules_check.cpp holds it
// against the rules as the entry points checked them one by one).
#pragma once
#include "../../include/str_er.h"

#include <stdint.h>

namespace str_er_host {

// what a detect call is, as far as the flags care
struct CallShape {
    bool frames;          // frames of an image: the text and line maps are possible
    bool all_planes;      // every plane of an image (planes_per_image > 0): track / group are possible
    bool strip;           // str_er_strip_merge_ex
    bool subset;          // str_er_detect_bgr_planes: a plane_select subset of the frames' planes
};

struct StageVerdict {
    int         code;     // STR_ER_OK or the error
    const char *msg;      // why (null when OK)
};

// cascades: both cascades loaded; svm1800: an SVM model loaded with dim = 1800; lexicon: a lexicon set (str_er_set_lexicon); bigram: a bigram
// table set (str_er_set_bigram).  The first rule that fails decides; the call's shape comes first.
inline StageVerdict check_stages(uint32_t st, const CallShape &k, bool cascades, bool svm1800, bool lexicon = false, bool bigram = false)
{
    auto any = [st](uint32_t f) { return (st & f) != 0; };
    const uint32_t maps = STR_ER_WANT_TEXT_MAP | STR_ER_WANT_LINE_MAP, crops = STR_ER_WANT_LINE_CROPS | STR_ER_WANT_LINE_GLYPHS;
    const uint32_t sup = STR_ER_GROUP_INNER_SUP | STR_ER_GROUP_OVERLAP_SUP;
    struct Rule { bool bad; int code; const char *msg; };
    const Rule rules[] = {
        // STR_ER_WANT_TRACK_DECODE rides on STR_ER_WANT_LINE_LINKS (the text tracks) and on STR_ER_WANT_WORD_DECODE (the rows, the seeds'
        // strings and the table), and through the latter on STR_ER_WANT_RUN_READ: refused without either and where either is refused,
        // first of all, so that the refusal names this flag (the table rule stays the decoder's, below); it needs neither
        // STR_ER_WANT_WORD_MATCH nor a lexicon; a call without the flag meets no new rule
        {k.strip && any(STR_ER_WANT_TRACK_DECODE), STR_ER_EINVAL, "STR_ER_WANT_TRACK_DECODE is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_TRACK_DECODE), STR_ER_EINVAL, "STR_ER_WANT_TRACK_DECODE needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_TRACK_DECODE) && !any(STR_ER_WANT_LINE_LINKS), STR_ER_EINVAL, "STR_ER_WANT_TRACK_DECODE needs STR_ER_WANT_LINE_LINKS"},
        {any(STR_ER_WANT_TRACK_DECODE) && !any(STR_ER_WANT_WORD_DECODE), STR_ER_EINVAL, "STR_ER_WANT_TRACK_DECODE needs STR_ER_WANT_WORD_DECODE"},
        {any(STR_ER_WANT_TRACK_DECODE) && !any(STR_ER_WANT_RUN_READ), STR_ER_EINVAL,
         "STR_ER_WANT_TRACK_DECODE needs STR_ER_WANT_RUN_READ (through STR_ER_WANT_WORD_DECODE)"},
        // STR_ER_WANT_LATTICE_TRACK rides on STR_ER_WANT_TRACK_READ (the word tracks) and on STR_ER_WANT_LATTICE_MATCH (the lattices, the
        // rows and the lexicon), and through them on STR_ER_WANT_RUN_SPLIT, _WORD_MATCH, _LINE_LINKS and _RUN_READ: refused without any
        // of them and where they are refused, first of all, so that the refusal names this flag (the lexicon rule stays the matcher's,
        // below); a call without the flag meets no new rule
        {k.strip && any(STR_ER_WANT_LATTICE_TRACK), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_TRACK is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_LATTICE_TRACK), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_TRACK needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_LATTICE_TRACK) && !any(STR_ER_WANT_TRACK_READ), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_TRACK needs STR_ER_WANT_TRACK_READ"},
        {any(STR_ER_WANT_LATTICE_TRACK) && !any(STR_ER_WANT_LATTICE_MATCH), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_TRACK needs STR_ER_WANT_LATTICE_MATCH"},
        {any(STR_ER_WANT_LATTICE_TRACK) && !any(STR_ER_WANT_RUN_SPLIT), STR_ER_EINVAL,
         "STR_ER_WANT_LATTICE_TRACK needs STR_ER_WANT_RUN_SPLIT (through STR_ER_WANT_LATTICE_MATCH)"},
        {any(STR_ER_WANT_LATTICE_TRACK) && !any(STR_ER_WANT_WORD_MATCH), STR_ER_EINVAL,
         "STR_ER_WANT_LATTICE_TRACK needs STR_ER_WANT_WORD_MATCH (through STR_ER_WANT_TRACK_READ and STR_ER_WANT_LATTICE_MATCH)"},
        {any(STR_ER_WANT_LATTICE_TRACK) && !any(STR_ER_WANT_LINE_LINKS), STR_ER_EINVAL,
         "STR_ER_WANT_LATTICE_TRACK needs STR_ER_WANT_LINE_LINKS (through STR_ER_WANT_TRACK_READ)"},
        {any(STR_ER_WANT_LATTICE_TRACK) && !any(STR_ER_WANT_RUN_READ), STR_ER_EINVAL,
         "STR_ER_WANT_LATTICE_TRACK needs STR_ER_WANT_RUN_READ (through STR_ER_WANT_RUN_SPLIT and STR_ER_WANT_WORD_MATCH)"},
        // STR_ER_WANT_TRACK_READ rides on STR_ER_WANT_LINE_LINKS (the text tracks) and on STR_ER_WANT_WORD_MATCH (the cost rows and the
        // lexicon): refused without either and where either is refused, first of all, so that the refusal names this flag; a call
        // without the flag meets no new rule
        {k.strip && any(STR_ER_WANT_TRACK_READ), STR_ER_EINVAL, "STR_ER_WANT_TRACK_READ is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_TRACK_READ), STR_ER_EINVAL, "STR_ER_WANT_TRACK_READ needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_TRACK_READ) && !any(STR_ER_WANT_LINE_LINKS), STR_ER_EINVAL, "STR_ER_WANT_TRACK_READ needs STR_ER_WANT_LINE_LINKS"},
        {any(STR_ER_WANT_TRACK_READ) && !any(STR_ER_WANT_WORD_MATCH), STR_ER_EINVAL, "STR_ER_WANT_TRACK_READ needs STR_ER_WANT_WORD_MATCH"},
        // STR_ER_WANT_LATTICE_MATCH rides on STR_ER_WANT_RUN_SPLIT (the lattice) and on STR_ER_WANT_WORD_MATCH (the rows and the lexicon):
        // refused without either and where either is refused, ahead of those flags' rules, so that the refusal names this flag (the
        // lexicon rule stays the matcher's, below); a call without the flag meets no new rule
        {k.strip && any(STR_ER_WANT_LATTICE_MATCH), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_MATCH is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_LATTICE_MATCH), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_MATCH needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_LATTICE_MATCH) && !any(STR_ER_WANT_RUN_SPLIT), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_MATCH needs STR_ER_WANT_RUN_SPLIT"},
        {any(STR_ER_WANT_LATTICE_MATCH) && !any(STR_ER_WANT_WORD_MATCH), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_MATCH needs STR_ER_WANT_WORD_MATCH"},
        {any(STR_ER_WANT_LATTICE_MATCH) && !any(STR_ER_WANT_RUN_READ), STR_ER_EINVAL,
         "STR_ER_WANT_LATTICE_MATCH needs STR_ER_WANT_RUN_READ (through STR_ER_WANT_RUN_SPLIT and STR_ER_WANT_WORD_MATCH)"},
        // STR_ER_WANT_LATTICE_DECODE rides on STR_ER_WANT_RUN_SPLIT (and through it on STR_ER_WANT_RUN_READ): refused without it and where
        // it is refused, ahead of that flag's rules, so that the refusal names this flag (its table rule is with the models' below); a
        // call without the flag meets no new rule
        {k.strip && any(STR_ER_WANT_LATTICE_DECODE), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_DECODE is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_LATTICE_DECODE), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_DECODE needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_LATTICE_DECODE) && !any(STR_ER_WANT_RUN_SPLIT), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_DECODE needs STR_ER_WANT_RUN_SPLIT"},
        {any(STR_ER_WANT_LATTICE_DECODE) && !any(STR_ER_WANT_RUN_READ), STR_ER_EINVAL, "STR_ER_WANT_LATTICE_DECODE needs STR_ER_WANT_RUN_READ (through STR_ER_WANT_RUN_SPLIT)"},
        // STR_ER_WANT_RUN_SPLIT rides on STR_ER_WANT_RUN_READ as STR_ER_WANT_WORD_MATCH does; its parameters have defaults, so it needs no
        // state of the context; a call without the flag meets no new rule
        {k.strip && any(STR_ER_WANT_RUN_SPLIT), STR_ER_EINVAL, "STR_ER_WANT_RUN_SPLIT is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_RUN_SPLIT), STR_ER_EINVAL, "STR_ER_WANT_RUN_SPLIT needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_RUN_SPLIT) && !any(STR_ER_WANT_RUN_READ), STR_ER_EINVAL, "STR_ER_WANT_RUN_SPLIT needs STR_ER_WANT_RUN_READ"},
        // STR_ER_WANT_WORD_DECODE rides on STR_ER_WANT_RUN_READ as STR_ER_WANT_WORD_MATCH does (its table rule is with the models' below);
        // a call without the flag meets no new rule
        {k.strip && any(STR_ER_WANT_WORD_DECODE), STR_ER_EINVAL, "STR_ER_WANT_WORD_DECODE is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_WORD_DECODE), STR_ER_EINVAL, "STR_ER_WANT_WORD_DECODE needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_WORD_DECODE) && !any(STR_ER_WANT_RUN_READ), STR_ER_EINVAL, "STR_ER_WANT_WORD_DECODE needs STR_ER_WANT_RUN_READ"},
        // STR_ER_WANT_WORD_MATCH rides on STR_ER_WANT_RUN_READ: refused without it and where it is refused, first of all, so that the
        // refusal names this flag (its lexicon rule is with the models' below); a call without the flag meets no new rule
        {k.strip && any(STR_ER_WANT_WORD_MATCH), STR_ER_EINVAL, "STR_ER_WANT_WORD_MATCH is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_WORD_MATCH), STR_ER_EINVAL, "STR_ER_WANT_WORD_MATCH needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_WORD_MATCH) && !any(STR_ER_WANT_RUN_READ), STR_ER_EINVAL, "STR_ER_WANT_WORD_MATCH needs STR_ER_WANT_RUN_READ"},
        // STR_ER_WANT_RUN_READ rides on STR_ER_WANT_LINE_WORDS: refused without it and where it is refused, with a message that names
        // this flag (its model rule is with STR_ER_STAGE_OCR_LINES' below); a call without the flag meets no new rule
        {k.strip && any(STR_ER_WANT_RUN_READ), STR_ER_EINVAL, "STR_ER_WANT_RUN_READ is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_RUN_READ), STR_ER_EINVAL, "STR_ER_WANT_RUN_READ needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_RUN_READ) && !any(STR_ER_WANT_LINE_WORDS), STR_ER_EINVAL, "STR_ER_WANT_RUN_READ needs STR_ER_WANT_LINE_WORDS"},
        // STR_ER_WANT_LINE_WORDS rides on STR_ER_WANT_FRAME_LINES as the two flags below do
        {k.strip && any(STR_ER_WANT_LINE_WORDS), STR_ER_EINVAL, "STR_ER_WANT_LINE_WORDS is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_LINE_WORDS), STR_ER_EINVAL, "STR_ER_WANT_LINE_WORDS needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_LINE_WORDS) && !any(STR_ER_WANT_FRAME_LINES), STR_ER_EINVAL, "STR_ER_WANT_LINE_WORDS needs STR_ER_WANT_FRAME_LINES"},
        // STR_ER_WANT_LINE_GEOM rides on STR_ER_WANT_FRAME_LINES in the same way: refused without it and where it is refused, with a
        // message that names this flag; with it the flag changes no verdict
        {k.strip && any(STR_ER_WANT_LINE_GEOM), STR_ER_EINVAL, "STR_ER_WANT_LINE_GEOM is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_LINE_GEOM), STR_ER_EINVAL, "STR_ER_WANT_LINE_GEOM needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_LINE_GEOM) && !any(STR_ER_WANT_FRAME_LINES), STR_ER_EINVAL, "STR_ER_WANT_LINE_GEOM needs STR_ER_WANT_FRAME_LINES"},
        // STR_ER_WANT_LINE_LINKS rides on STR_ER_WANT_FRAME_LINES: refused without it and where it is refused, first of all, so that the
        // refusal names this flag; with it the flag changes no verdict
        {k.strip && any(STR_ER_WANT_LINE_LINKS), STR_ER_EINVAL, "STR_ER_WANT_LINE_LINKS is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_LINE_LINKS), STR_ER_EINVAL, "STR_ER_WANT_LINE_LINKS needs frames (not the per-plane calls)"},
        {any(STR_ER_WANT_LINE_LINKS) && !any(STR_ER_WANT_FRAME_LINES), STR_ER_EINVAL, "STR_ER_WANT_LINE_LINKS needs STR_ER_WANT_FRAME_LINES"},
        // the call's shape
        {k.subset && any(STR_ER_STAGE_TRACK | STR_ER_STAGE_GROUP | STR_ER_STAGE_OCR_LINES), STR_ER_EINVAL,
         "er_track / er_grouping read every plane of an image: not with a plane subset"},
        {k.strip && any(STR_ER_WANT_MASKS), STR_ER_EINVAL, "STR_ER_WANT_MASKS is not supported by the strip path (str_er_strip_merge)"},
        {k.strip && any(STR_ER_WANT_SHAPES), STR_ER_EINVAL, "STR_ER_WANT_SHAPES is not supported by the strip path (str_er_strip_merge)"},
        {k.strip && any(STR_ER_WANT_STROKES), STR_ER_EINVAL, "STR_ER_WANT_STROKES is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(maps), STR_ER_EINVAL, "STR_ER_WANT_TEXT_MAP / _LINE_MAP need frames (not the per-plane calls or the strip path)"},
        {k.strip && any(crops), STR_ER_EINVAL, "STR_ER_WANT_LINE_CROPS / _GLYPHS are not supported by the strip path (str_er_strip_merge)"},
        {k.strip && any(STR_ER_WANT_FRAME_LINES), STR_ER_EINVAL, "STR_ER_WANT_FRAME_LINES is not supported by the strip path (str_er_strip_merge)"},
        {!k.frames && any(STR_ER_WANT_FRAME_LINES), STR_ER_EINVAL, "STR_ER_WANT_FRAME_LINES needs frames (not the per-plane calls)"},
        // the maps (sized before anything of a frame call is enqueued: ahead of the state of the context)
        {any(STR_ER_WANT_TEXT_MAP) && !any(STR_ER_STAGE_CLASSIFY), STR_ER_EINVAL, "STR_ER_WANT_TEXT_MAP needs STR_ER_STAGE_CLASSIFY"},
        {any(STR_ER_WANT_LINE_MAP) && !any(STR_ER_STAGE_GROUP), STR_ER_EINVAL, "STR_ER_WANT_LINE_MAP needs STR_ER_STAGE_GROUP"},
        {any(STR_ER_WANT_FRAME_LINES) && !any(STR_ER_STAGE_GROUP), STR_ER_EINVAL, "STR_ER_WANT_FRAME_LINES needs STR_ER_STAGE_GROUP"},
        // the stages, each behind what it needs
        {any(STR_ER_STAGE_CLASSIFY) && !cascades, STR_ER_ESTATE, "classify needs both cascades (str_er_load_cascade)"},
        {!any(STR_ER_STAGE_EXTRACT), STR_ER_EINVAL, "stages must include STR_ER_STAGE_EXTRACT"},
        {any(STR_ER_STAGE_CLASSIFY) && !any(STR_ER_STAGE_NMS), STR_ER_EINVAL, "STR_ER_STAGE_CLASSIFY needs STR_ER_STAGE_NMS"},
        {any(STR_ER_STAGE_OCR) && !any(STR_ER_STAGE_CLASSIFY), STR_ER_EINVAL, "STR_ER_STAGE_OCR needs STR_ER_STAGE_CLASSIFY"},
        {any(STR_ER_STAGE_OCR) && !svm1800, STR_ER_ESTATE, "STR_ER_STAGE_OCR needs an SVM model loaded with dim = 1800 (str_er_load_svm_model)"},
        {any(STR_ER_STAGE_TRACK) && !any(STR_ER_STAGE_CLASSIFY), STR_ER_EINVAL, "STR_ER_STAGE_TRACK needs STR_ER_STAGE_CLASSIFY"},
        {any(STR_ER_STAGE_GROUP | sup) && !any(STR_ER_STAGE_TRACK), STR_ER_EINVAL, "STR_ER_STAGE_GROUP needs STR_ER_STAGE_TRACK"},
        {any(sup) && !any(STR_ER_STAGE_GROUP), STR_ER_EINVAL, "STR_ER_GROUP_INNER_SUP / _OVERLAP_SUP modify STR_ER_STAGE_GROUP"},
        {any(STR_ER_STAGE_OCR_LINES) && !any(STR_ER_STAGE_GROUP), STR_ER_EINVAL, "STR_ER_STAGE_OCR_LINES needs STR_ER_STAGE_GROUP"},
        {any(crops) && !any(STR_ER_STAGE_GROUP), STR_ER_EINVAL, "STR_ER_WANT_LINE_CROPS / _GLYPHS need STR_ER_STAGE_GROUP"},
        {any(STR_ER_WANT_LINE_GLYPHS) && !any(STR_ER_WANT_LINE_CROPS), STR_ER_EINVAL, "STR_ER_WANT_LINE_GLYPHS needs STR_ER_WANT_LINE_CROPS"},
        {any(STR_ER_STAGE_OCR_LINES) && !svm1800, STR_ER_ESTATE,
         "STR_ER_STAGE_OCR_LINES needs an SVM model loaded with dim = 1800 (str_er_load_svm_model)"},
        {any(STR_ER_WANT_RUN_READ) && !svm1800, STR_ER_ESTATE,
         "STR_ER_WANT_RUN_READ needs an SVM model loaded with dim = 1800 (str_er_load_svm_model)"},
        {any(STR_ER_WANT_WORD_MATCH) && !lexicon, STR_ER_ESTATE, "STR_ER_WANT_WORD_MATCH needs a lexicon (str_er_set_lexicon)"},
        {any(STR_ER_WANT_WORD_DECODE) && !bigram, STR_ER_ESTATE, "STR_ER_WANT_WORD_DECODE needs a bigram table (str_er_set_bigram)"},
        {any(STR_ER_WANT_LATTICE_DECODE) && !bigram, STR_ER_ESTATE, "STR_ER_WANT_LATTICE_DECODE needs a bigram table (str_er_set_bigram)"},
        {any(STR_ER_STAGE_TRACK) && !k.all_planes, STR_ER_EINVAL, "STR_ER_STAGE_TRACK needs BGR frames (calc_color reads the YCrCb image)"},
    };
    for (const Rule &r : rules)
        if (r.bad) return {r.code, r.msg};
    return {STR_ER_OK, nullptr};
}

// The track decode over the members' piece lattices (str_er_lattice_track_decode) has no flag of its own: it is a setting of the context
// (str_er_set_lattice_track_decode) and runs in a detect call that carries both STR_ER_WANT_TRACK_DECODE and STR_ER_WANT_LATTICE_DECODE,
// whose rules above already bring the word tracks, the lattice rows and the table.  With either flag missing the setting does nothing.
inline bool lattice_track_decode_runs(uint32_t st, bool setting)
{
    return setting && (st & STR_ER_WANT_TRACK_DECODE) != 0 && (st & STR_ER_WANT_LATTICE_DECODE) != 0;
}

} // namespace str_er_host
