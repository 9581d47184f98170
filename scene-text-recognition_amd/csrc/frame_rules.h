// frame_rules.h -- INTERNAL: what a source frame (or plane) in the caller's memory is: the bytes of a row, the rows of a frame, and which
// str_er_image_ref a list call or a list submission of the ingest stream accepts.  HIP-free and header-only; tests/cpp/frame_rules_check.cpp.
#pragma once
#include "../../include/str_er.h"
#include <string>

namespace str_er_host {

// BGR: interleaved 8UC3.  NV12: h rows of luma, then h / 2 rows of interleaved chroma, `stride` bytes per row both; w, h even.  PLANE: 8 bit.
enum class SrcFormat { BGR, NV12, PLANE };

inline int64_t src_row_bytes(int32_t w, SrcFormat f) { return f == SrcFormat::BGR ? (int64_t)w * 3 : (int64_t)w; }
inline int64_t src_rows(int32_t h, SrcFormat f) { return f == SrcFormat::NV12 ? (int64_t)h + h / 2 : (int64_t)h; }

// One frame of a list: `name` is "frame 3" or "plane 0", `owner` whose capacity max_w x max_h is.  STR_ER_OK, or the code with `msg` written.
inline int check_image_ref(const str_er_image_ref &r, SrcFormat f, const std::string &name, int32_t max_w, int32_t max_h, const char *owner, std::string &msg)
{
    if (!r.data) msg = name + ": null data";
    else if (r.w < 1 || r.h < 1) msg = name + ": empty";
    else if (r.stride < src_row_bytes(r.w, f)) msg = name + ": stride smaller than a row";
    else if (r.stride > 0x7FFFFFFF) msg = name + ": stride too large";
    else if (f == SrcFormat::NV12 && ((r.w | r.h) & 1)) msg = name + ": NV12 frames have even width and height";
    else if (r.w > max_w || r.h > max_h) {
        msg = name + ": " + std::to_string(r.w) + " x " + std::to_string(r.h) + " larger than " + owner + " " + std::to_string(max_w) + " x " + std::to_string(max_h);
        return STR_ER_ECAPACITY;
    } else return STR_ER_OK;
    return STR_ER_EINVAL;
}

} // namespace str_er_host
