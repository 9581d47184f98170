// word_match_rules.h -- INTERNAL: the rules of the lexicon matcher (the contract is at str_er_word_match in str_er.h): the threshold
// table, cost(), the cost row of a run, the edit distance of a word's runs against one entry and the best / second merge.  HIP-free and
// header-only: the host entry points (api_word_match.cpp: str_er_cost_thresholds, str_er_prob_costs, the single-thread matcher of
// tools/dev_word_match.py) and tests/cpp/word_match_rules_check.cpp use this same code; word_match_kernels.hip states the same rules
// for the device and is held against the numpy reference (tests/word_match_ref.py), which is written from the definition.
#pragma once
#include "../../include/str_er.h"

#include <math.h>
#include <stdint.h>

namespace str_er_wm {

constexpr int ALPHABET = 65;        // the characters of str_er_ocr_char
constexpr int MAX_LEN = 32;         // bytes of an entry, runs of a word that is tried
constexpr int MAX_ENTRIES = 1 << 20;
constexpr int N_THRESH = 255;
constexpr uint64_t NO_KEY = ~0ull;  // "no entry" of a best / second pair

// the eight doubles nearest to 2^(-j/8)
constexpr double MANTISSA[8] = {0x1.0000000000000p+0, 0x1.d5818dcfba487p-1, 0x1.ae89f995ad3adp-1, 0x1.8ace5422aa0dbp-1,
                                0x1.6a09e667f3bcdp-1, 0x1.4bfdad5362a27p-1, 0x1.306fe0a31b715p-1, 0x1.172b83c7d517bp-1};

// T[c] = MANTISSA[c % 8] * 2^-(c / 8), c = 0 .. 254: exact (a power of two times a normal number, far from the subnormals)
inline void thresholds(double T[N_THRESH])
{
    for (int c = 0; c < N_THRESH; ++c) T[c] = ldexp(MANTISSA[c % 8], -(c / 8));
}

// the smallest c with p >= T[c], else 255 (NaN and negative p: no comparison holds).  T falls with c: a bisection of comparisons only.
inline uint8_t cost(double p, const double T[N_THRESH])
{
    if (!(p >= T[N_THRESH - 1])) return 255;
    int lo = 0, hi = N_THRESH - 1;          // the answer is in [lo, hi]; p >= T[hi]
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (p >= T[mid]) hi = mid; else lo = mid + 1;
    }
    return (uint8_t)lo;
}

// the other letter of a case pair ('A' + i = label 10 + i, 'a' + i = label 36 + i), or a itself
inline int fold_partner(int a) { return a >= 10 && a < 36 ? a + 26 : a >= 36 && a < 62 ? a - 26 : a; }

// The cost row of a run from the k class probabilities of a model with the given labels: C[a] = cost(prob[j]) for the class j with
// label a (the first such class where a model names a label twice), 255 without one; labels outside 0 .. 64 are ignored.
inline void cost_row(const double *prob, int k, const int32_t *labels, bool fold, const double T[N_THRESH], uint8_t C[ALPHABET])
{
    bool seen[ALPHABET] = {};
    for (int a = 0; a < ALPHABET; ++a) C[a] = 255;
    for (int j = 0; j < k; ++j) {
        const int32_t a = labels[j];
        if (a < 0 || a >= ALPHABET || seen[a]) continue;
        seen[a] = true;
        C[a] = cost(prob[j], T);
    }
    if (fold)
        for (int a = 10; a < 36; ++a) C[a] = C[a + 26] = C[a] < C[a + 26] ? C[a] : C[a + 26];
}

// the label of a character of the alphabet ("0123456789A..Za..z&()"), -1 for any other byte
inline int char_label(unsigned char ch)
{
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'A' && ch <= 'Z') return 10 + (ch - 'A');
    if (ch >= 'a' && ch <= 'z') return 36 + (ch - 'a');
    return ch == '&' ? 62 : ch == '(' ? 63 : ch == ')' ? 64 : -1;
}

// what str_er_set_lexicon takes: STR_ER_OK, or the code and why
inline int lexicon_check(const char *bytes, const int32_t *offsets, int32_t n, uint32_t flags, const char **why)
{
    const auto bad = [&](int code, const char *msg) { if (why) *why = msg; return code; };
    if (n < 0 || (flags & ~STR_ER_LEXICON_FOLD_CASE)) return bad(STR_ER_EINVAL, "lexicon: bad arguments");
    if (n > MAX_ENTRIES) return bad(STR_ER_ECAPACITY, "lexicon: more than 2^20 entries");
    if (n == 0) return STR_ER_OK;
    if (!bytes || !offsets || offsets[0] != 0) return bad(STR_ER_EINVAL, "lexicon: the offsets do not start at 0");
    for (int32_t e = 0; e < n; ++e) {
        const int64_t len = (int64_t)offsets[e + 1] - offsets[e];
        if (len < 1 || len > MAX_LEN) return bad(STR_ER_EINVAL, "lexicon: an entry of length 0 or above 32 (or offsets that do not lie back to back)");
        for (int32_t i = offsets[e]; i < offsets[e + 1]; ++i)
            if (char_label((unsigned char)bytes[i]) < 0) return bad(STR_ER_EINVAL, "lexicon: a byte outside the alphabet of str_er_ocr_char");
    }
    return STR_ER_OK;
}

struct MatchParams { int32_t ins = 64, del = 64, band = 2; };

inline bool params_ok(int32_t ins, int32_t del, int32_t band) { return ins >= 1 && ins <= 255 && del >= 1 && del <= 255 && band >= 0 && band <= 31; }
inline bool in_band(int m, int len, int band) { return m <= MAX_LEN && (len > m ? len - m : m - len) <= band; }

// D[m][len] of the entry e (labels 0 .. 64) for the m <= 32 cost rows C (65 bytes each, back to back); fold: both letters of a case
// pair count as the cheaper of the two
inline int32_t entry_cost(const uint8_t *C, int m, const uint8_t *e, int len, int32_t ins, int32_t del, bool fold)
{
    int32_t col[MAX_LEN + 1];                // D[i][j - 1], then D[i][j], over the runs i
    for (int i = 0; i <= m; ++i) col[i] = i * del;
    for (int j = 1; j <= len; ++j) {
        const int a = e[j - 1], b = fold ? fold_partner(a) : a;
        int32_t diag = col[0];
        col[0] = j * ins;
        for (int i = 1; i <= m; ++i) {
            const uint8_t *row = C + (size_t)(i - 1) * ALPHABET;
            const int32_t  sub = diag + (row[a] < row[b] ? row[a] : row[b]), up = col[i - 1] + del, left = col[i] + ins;
            diag = col[i];
            col[i] = sub < up ? (sub < left ? sub : left) : (up < left ? up : left);
        }
    }
    return col[m];
}

inline uint64_t make_key(int32_t cost, int32_t index) { return (uint64_t)(uint32_t)cost << 32 | (uint32_t)index; }

// the two smallest keys seen so far (keys of different entries differ)
struct Best2 {
    uint64_t k1 = NO_KEY, k2 = NO_KEY;
    void add(uint64_t k)
    {
        if (k < k1) { k2 = k1; k1 = k; }
        else if (k < k2) k2 = k;
    }
    void merge(const Best2 &o) { add(o.k1); add(o.k2); }
};

inline int32_t free_cost(const uint8_t *C, int m)
{
    int32_t s = 0;
    for (int i = 0; i < m; ++i) {
        uint8_t lo = 255;
        for (int a = 0; a < ALPHABET; ++a) lo = C[(size_t)i * ALPHABET + a] < lo ? C[(size_t)i * ALPHABET + a] : lo;
        s += lo;
    }
    return s;
}

inline str_er_word_match make_match(const Best2 &b, int32_t free_c, int32_t n_tried)
{
    str_er_word_match r;
    r.entry = b.k1 == NO_KEY ? -1 : (int32_t)(uint32_t)b.k1;
    r.cost = b.k1 == NO_KEY ? -1 : (int32_t)(b.k1 >> 32);
    r.second_entry = b.k2 == NO_KEY ? -1 : (int32_t)(uint32_t)b.k2;
    r.second_cost = b.k2 == NO_KEY ? -1 : (int32_t)(b.k2 >> 32);
    r.free_cost = free_c;
    r.n_tried = n_tried;
    return r;
}

// one word against the whole lexicon (entries as labels, offsets[n + 1]), on one thread
inline str_er_word_match match_word(const uint8_t *C, int m, const uint8_t *labels, const int32_t *offsets, int32_t n, const MatchParams &p, bool fold)
{
    Best2   b;
    int32_t tried = 0;
    for (int32_t e = 0; e < n; ++e) {
        const int len = offsets[e + 1] - offsets[e];
        if (!in_band(m, len, p.band)) continue;
        ++tried;
        b.add(make_key(entry_cost(C, m, labels + offsets[e], len, p.ins, p.del, fold), e));
    }
    return make_match(b, free_cost(C, m), tried);
}

} // namespace str_er_wm
