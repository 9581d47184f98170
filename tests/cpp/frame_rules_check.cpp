// Host-only check of csrc/frame_rules.h (compiled and run by tests/test_host_cpp.py): the bytes of a source row and the rows of a source frame
// for BGR, NV12 and single planes, and check_image_ref -- every rejection with its code and message, in the order the
// rules are stated (an earlier rule wins), and the edges that must pass: 1 x 1, a 2 x 2 NV12 frame, a stride of exactly one row, a stride
// of 0x7FFFFFFF, a frame of exactly the capacity.
#include <stdio.h>
#include <string>

#include "frame_rules.h"

using namespace str_er_host;

static int bad = 0;
static const uint8_t px[16] = {0};

static void expect(const char *what, const str_er_image_ref &r, SrcFormat f, const char *name, const char *owner, int code, const char *msg)
{
    std::string got = "untouched";
    const int rc = check_image_ref(r, f, name, 640, 480, owner, got);
    if (rc != code || (code != STR_ER_OK && got != msg) || (code == STR_ER_OK && got != "untouched")) {
        fprintf(stderr, "%s: code %d (expected %d), message \"%s\" (expected \"%s\")\n", what, rc, code, got.c_str(), msg);
        ++bad;
    }
}

#define EQ(a, b) do { if ((int64_t)(a) != (int64_t)(b)) { fprintf(stderr, "line %d: %s = %lld, expected %lld\n", __LINE__, #a, (long long)(a), (long long)(b)); ++bad; } } while (0)

int main()
{
    const SrcFormat BGR = SrcFormat::BGR, NV12 = SrcFormat::NV12, PLANE = SrcFormat::PLANE;
    // rows and row bytes
    EQ(src_row_bytes(1, BGR), 3); EQ(src_row_bytes(1, NV12), 1); EQ(src_row_bytes(1, PLANE), 1);
    EQ(src_row_bytes(1920, BGR), 5760); EQ(src_row_bytes(1920, NV12), 1920); EQ(src_row_bytes(65535, BGR), 196605);
    EQ(src_row_bytes(0x7FFFFFFF, BGR), 3 * (int64_t)0x7FFFFFFF);               // (64-bit: no wrap at 3 w)
    EQ(src_rows(1, BGR), 1); EQ(src_rows(1, PLANE), 1); EQ(src_rows(2, NV12), 3); EQ(src_rows(1080, NV12), 1620); EQ(src_rows(1080, BGR), 1080);
    EQ(src_rows(0x7FFFFFFE, NV12), (int64_t)0x7FFFFFFE + 0x3FFFFFFF);

    const char *ctx = "the context capacity", *str = "the stream's capacity";
    // every rejection
    expect("null data", {nullptr, 10, 10, 30}, BGR, "frame 1", ctx, STR_ER_EINVAL, "frame 1: null data");
    expect("zero width", {px, 0, 10, 30}, BGR, "frame 0", ctx, STR_ER_EINVAL, "frame 0: empty");
    expect("zero height", {px, 10, 0, 30}, PLANE, "plane 2", ctx, STR_ER_EINVAL, "plane 2: empty");
    expect("negative size", {px, -1, -1, 30}, NV12, "frame 0", str, STR_ER_EINVAL, "frame 0: empty");
    expect("BGR stride one short", {px, 100, 100, 299}, BGR, "frame 1", ctx, STR_ER_EINVAL, "frame 1: stride smaller than a row");
    expect("NV12 stride one short", {px, 100, 100, 99}, NV12, "frame 1", str, STR_ER_EINVAL, "frame 1: stride smaller than a row");
    expect("plane stride one short", {px, 50, 50, 49}, PLANE, "plane 0", ctx, STR_ER_EINVAL, "plane 0: stride smaller than a row");
    expect("negative stride", {px, 2, 2, -6}, BGR, "frame 0", ctx, STR_ER_EINVAL, "frame 0: stride smaller than a row");
    expect("stride 2^31", {px, 2, 2, (int64_t)0x80000000LL}, BGR, "frame 0", ctx, STR_ER_EINVAL, "frame 0: stride too large");
    expect("stride 2^31, stream", {px, 2, 2, (int64_t)0x80000000LL}, NV12, "frame 7", str, STR_ER_EINVAL, "frame 7: stride too large");
    expect("NV12 odd width", {px, 3, 2, 3}, NV12, "frame 0", ctx, STR_ER_EINVAL, "frame 0: NV12 frames have even width and height");
    expect("NV12 odd height", {px, 2, 3, 2}, NV12, "frame 0", str, STR_ER_EINVAL, "frame 0: NV12 frames have even width and height");
    expect("NV12 1 x 1", {px, 1, 1, 1}, NV12, "frame 0", ctx, STR_ER_EINVAL, "frame 0: NV12 frames have even width and height");
    expect("too wide", {px, 641, 200, 1923}, BGR, "frame 1", ctx, STR_ER_ECAPACITY, "frame 1: 641 x 200 larger than the context capacity 640 x 480");
    expect("too tall", {px, 100, 481, 300}, BGR, "frame 0", str, STR_ER_ECAPACITY, "frame 0: 100 x 481 larger than the stream's capacity 640 x 480");
    expect("plane too wide", {px, 641, 1, 641}, PLANE, "plane 3", ctx, STR_ER_ECAPACITY, "plane 3: 641 x 1 larger than the context capacity 640 x 480");
    // an earlier rule wins
    expect("null before empty", {nullptr, 0, 0, 0}, BGR, "frame 0", ctx, STR_ER_EINVAL, "frame 0: null data");
    expect("empty before stride", {px, 0, 5, -1}, BGR, "frame 0", ctx, STR_ER_EINVAL, "frame 0: empty");
    expect("stride before parity", {px, 3, 3, 2}, NV12, "frame 0", ctx, STR_ER_EINVAL, "frame 0: stride smaller than a row");
    expect("stride before capacity", {px, 700, 500, 2099}, BGR, "frame 0", ctx, STR_ER_EINVAL, "frame 0: stride smaller than a row");
    expect("parity before capacity", {px, 701, 500, 701}, NV12, "frame 0", ctx, STR_ER_EINVAL, "frame 0: NV12 frames have even width and height");
    // what passes
    expect("1 x 1 BGR", {px, 1, 1, 3}, BGR, "frame 0", ctx, STR_ER_OK, "");
    expect("1 x 1 plane", {px, 1, 1, 1}, PLANE, "plane 0", ctx, STR_ER_OK, "");
    expect("2 x 2 NV12", {px, 2, 2, 2}, NV12, "frame 0", str, STR_ER_OK, "");
    expect("stride exactly a row, BGR", {px, 100, 100, 300}, BGR, "frame 0", ctx, STR_ER_OK, "");
    expect("stride exactly a row, NV12", {px, 100, 100, 100}, NV12, "frame 0", ctx, STR_ER_OK, "");
    expect("stride exactly a row, plane", {px, 50, 50, 50}, PLANE, "plane 0", ctx, STR_ER_OK, "");
    expect("stride 2^31 - 1", {px, 2, 2, 0x7FFFFFFF}, BGR, "frame 0", ctx, STR_ER_OK, "");
    expect("stride 2^31 - 1, NV12", {px, 2, 2, 0x7FFFFFFF}, NV12, "frame 0", str, STR_ER_OK, "");
    expect("exactly the capacity", {px, 640, 480, 1920}, BGR, "frame 0", ctx, STR_ER_OK, "");
    expect("exactly the capacity, NV12", {px, 640, 480, 640}, NV12, "frame 0", str, STR_ER_OK, "");
    expect("odd BGR frame", {px, 211, 97, 633}, BGR, "frame 0", ctx, STR_ER_OK, "");

    if (bad) { printf("%d wrong\n", bad); return 1; }
    printf("frame rules ok\n");
    return 0;
}
