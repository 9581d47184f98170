// Host-only check of the STR_ER_WANT_LINE_GEOM rules of csrc/stage_rules.h (compiled and run by tests/test_line_geom_abi.py), for every
// combination of the other 19 flag bits, every call shape and both states of the context:
//   - without STR_ER_WANT_FRAME_LINES, without frames or on the strip path the flagged call is refused with STR_ER_EINVAL and a message
//     that names the flag;
//   - otherwise the flag changes nothing: the verdict (code and message) is that of the call without it.
#include <stdio.h>
#include <string.h>

#include "stage_rules.h"

using namespace str_er_host;

int main()
{
    static_assert(STR_ER_WANT_LINE_GEOM == (1u << 19), "the next free bit");
    long n = 0, refused = 0, bad = 0;
    for (int shape = 0; shape < 16; ++shape) {
        const CallShape k{(shape & 1) != 0, (shape & 2) != 0, (shape & 4) != 0, (shape & 8) != 0};
        for (int state = 0; state < 4; ++state)
            for (uint32_t st = 0; st < (1u << 19); ++st) {
                const StageVerdict plain = check_stages(st, k, (state & 1) != 0, (state & 2) != 0);
                const StageVerdict flag = check_stages(st | STR_ER_WANT_LINE_GEOM, k, (state & 1) != 0, (state & 2) != 0);
                ++n;
                bool ok;
                if (!k.frames || k.strip || !(st & STR_ER_WANT_FRAME_LINES)) {
                    ++refused;
                    ok = flag.code == STR_ER_EINVAL && flag.msg != nullptr && strstr(flag.msg, "STR_ER_WANT_LINE_GEOM") != nullptr;
                } else {
                    ok = flag.code == plain.code && ((flag.msg == nullptr && plain.msg == nullptr) || (flag.msg && plain.msg && !strcmp(flag.msg, plain.msg)));
                }
                if (!ok && bad++ < 10) fprintf(stderr, "shape %d state %d stages %u: plain %d, flagged %d (%s)\n", shape, state, st, plain.code, flag.code, flag.msg ? flag.msg : "");
            }
    }
    printf("%ld cases, %ld refused, %ld wrong\n", n, refused, bad);
    return bad ? 1 : 0;
}
