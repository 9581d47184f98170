// er_filter_hip.hpp -- C++ host-side mirror of the reference's `class ERFilter` hot-path
// surface (inc/ER.h:110-136), implemented on top of the C ABI in include/str_er.h.
//
// The reference keeps its host code in C++ and so does this: the class below has the same
// constructor arguments, public members and method names as the reference for the path
//
//     text_detect -> compute_channels -> er_tree_extract -> non_maximum_supression -> classify
//
// but takes plain 8-bit buffers instead of cv::Mat (OpenCV is not a dependency of this
// library).  A maintainer of the reference wraps `cv::Mat::data/step` in the `Image8` view
// below (see INTEGRATION.md for the exact patch).  `struct ER` / `ERs` keep the reference's
// field names (inc/ER.h:42-82) so downstream code (er_track, er_grouping, er_ocr,
// src/ER.cpp:532-786) compiles against it unchanged.
//
// Header-only; link with -lstr_er_hip.  Errors are reported the way the reference does for
// CV_Assert (src/ER.cpp:242): by throwing (std::runtime_error instead of cv::Exception).
#pragma once

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/str_er.h"

namespace str_er_host {

// Borrowed view of an 8-bit image: what cv::Mat gives through .data/.cols/.rows/.step.
struct Image8 {
    const uint8_t *data = nullptr;
    int cols = 0, rows = 0;
    int64_t step = 0;      // bytes per row
    int channels = 1;      // 1 (8UC1 plane) or 3 (8UC3, BGR)
    Image8() = default;
    Image8(const uint8_t *d, int c, int r, int64_t s, int ch) : data(d), cols(c), rows(r), step(s), channels(ch) {}
};

struct Rect { int x = 0, y = 0, width = 0, height = 0; int area() const { return width * height; } };
struct Point { int x = 0, y = 0; };

// Field-for-field the hot-path part of the reference's struct ER (inc/ER.h:42-80).
struct ER {
    int pixel = 0, level = 0, x = 0, y = 0;
    int area = 0;
    Rect bound;
    bool done = false;
    double stability = 0;
    ER *parent = nullptr, *child = nullptr, *next = nullptr;
    Point center;                                  // set by er_track (src/ER.cpp:542)
    double color1 = 0, color2 = 0, color3 = 0;     // set by er_track -> calc_color
    int ch = 0;
    // set by classify on pooled ERs (not in the reference, where strong/weak are separate lists)
    double score_strong = -DBL_MAX, score_weak = 0;
    uint32_t key = 0;
};
typedef std::vector<ER *> ERs;

// struct Text (inc/ER.h:84-97), the part er_grouping fills
struct Text {
    ERs ers;
    double slope = 0;
    Rect box;
};

// Owns the nodes of one plane's tree (the reference leaks them in image_mode and frees them
// with ERFilter::er_delete in video_mode, src/ER.cpp:194-233, src/utils.cpp:212-213).
struct ERTree {
    std::vector<ER> nodes;
    ER *root = nullptr;
};

class AdaBoostHandle {   // stands for `AdaBoost *stc, *wtc` (inc/ER.h:117-118): a loaded cascade file
public:
    explicit AdaBoostHandle(std::string path) : path_(std::move(path)) {}
    const std::string &path() const { return path_; }
private:
    std::string path_;
};

class ERFilter {
public:
    // inc/ER.h:113 -- same argument order and defaults
    ERFilter(int thresh_step = 2, int min_area = 100, int max_area = 100000, int stability_t = 2,
             double overlap_coef = 0.7, double min_ocr_prob = 0.01, int max_width = 1920, int max_height = 1080,
             int max_frames = 1, int device = 0)
        : MIN_OCR_PROB(min_ocr_prob)
    {
        str_er_params p;
        str_er_default_params(&p);
        p.thresh_step = thresh_step; p.min_area = min_area; p.max_area = max_area; p.stability_t = stability_t;
        p.overlap_coef = overlap_coef; p.max_width = max_width; p.max_height = max_height; p.max_frames = max_frames;
        p.device = device;
        str_er_ctx *c = nullptr;
        const int rc = str_er_create(&p, &c);
        if (rc != STR_ER_OK) throw std::runtime_error(std::string("str_er_create: ") + str_er_last_error(nullptr));
        ctx_.reset(c, str_er_destroy);
    }

    //! modules (inc/ER.h:116-119): assigning a cascade file loads it onto the GPU
    std::shared_ptr<AdaBoostHandle> stc, wtc;
    void set_stc(const std::string &file) { load(STR_ER_CASCADE_STRONG, file); stc = std::make_shared<AdaBoostHandle>(file); }
    void set_wtc(const std::string &file) { load(STR_ER_CASCADE_WEAK, file); wtc = std::make_shared<AdaBoostHandle>(file); }

    void set_thresh_step(int t) { check(str_er_set_thresh_step(ctx_.get(), t)); }   // src/ER.cpp:21-24
    void set_min_area(int m) { check(str_er_set_min_area(ctx_.get(), m)); }         // src/ER.cpp:27-30

    // ERFilter::text_detect up to classify (src/ER.cpp:33-60).  root/pool/strong/weak are resized to
    // the number of channels exactly like the reference does (:42-46); `all` stays empty unless
    // GET_ALL_ER semantics are wanted (inc/ER.h:24).  Returns the 7-slot times vector (:99-110).
    std::vector<double> text_detect(const Image8 &src, std::vector<ERTree> &trees, ERs &root, std::vector<ERs> &all,
                                    std::vector<ERs> &pool, std::vector<ERs> &strong, std::vector<ERs> &weak)
    {
        if (src.channels != 3) throw std::runtime_error("text_detect expects an 8UC3 BGR image");
        str_er_result *r = nullptr;
        check(str_er_detect_bgr(ctx_.get(), src.data, src.cols, src.rows, src.step, src.step * (int64_t)src.rows, 1,
                                STR_ER_MEM_HOST, STR_ER_STAGE_ALL | STR_ER_WANT_NODES, &r));
        std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
        const int n = str_er_result_n_planes(r);
        trees.assign(n, ERTree());
        root.assign(n, nullptr); all.assign(n, ERs()); pool.assign(n, ERs()); strong.assign(n, ERs()); weak.assign(n, ERs());
        for (int i = 0; i < n; ++i) unpack_plane(r, i, trees[i], pool[i], strong[i], weak[i]), root[i] = trees[i].root;
        const double *t = str_er_result_times(r);
        return std::vector<double>(t, t + 7);
    }

    // text_detect for a batch of 8UC3 BGR images of different sizes in one call (str_er_detect_bgr_list): what the reference's image
    // mode does one cv::imread at a time.  trees[f], root[f], pool[f], strong[f], weak[f] are what text_detect gives for frame f alone.
    // Returns the batch's 7-slot times vector.
    std::vector<double> text_detect_batch(const std::vector<Image8> &frames, std::vector<std::vector<ERTree>> &trees, std::vector<ERs> &root,
                                          std::vector<std::vector<ERs>> &pool, std::vector<std::vector<ERs>> &strong,
                                          std::vector<std::vector<ERs>> &weak)
    {
        std::vector<str_er_image_ref> refs(frames.size());
        for (size_t f = 0; f < frames.size(); ++f) {
            if (frames[f].channels != 3) throw std::runtime_error("text_detect_batch expects 8UC3 BGR images");
            refs[f].data = frames[f].data; refs[f].w = frames[f].cols; refs[f].h = frames[f].rows; refs[f].stride = frames[f].step;
        }
        str_er_result *r = nullptr;
        check(str_er_detect_bgr_list(ctx_.get(), refs.data(), (int32_t)refs.size(), STR_ER_MEM_HOST, STR_ER_STAGE_ALL | STR_ER_WANT_NODES, &r));
        std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
        return unpack_batch(r, frames.size(), trees, root, pool, strong, weak);
    }

    // The same for NV12 frames of different sizes (str_er_detect_nv12_list: what a hardware decoder delivers): frames[f] is an 8UC1
    // image of h + h/2 rows -- the luma plane, then the interleaved Cb/Cr rows -- of an even w x h frame.
    std::vector<double> text_detect_nv12_batch(const std::vector<Image8> &frames, std::vector<std::vector<ERTree>> &trees, std::vector<ERs> &root,
                                               std::vector<std::vector<ERs>> &pool, std::vector<std::vector<ERs>> &strong,
                                               std::vector<std::vector<ERs>> &weak)
    {
        std::vector<str_er_image_ref> refs(frames.size());
        for (size_t f = 0; f < frames.size(); ++f) {
            if (frames[f].channels != 1 || frames[f].rows % 3) throw std::runtime_error("text_detect_nv12_batch expects 8UC1 NV12 images of h + h/2 rows");
            refs[f].data = frames[f].data; refs[f].w = frames[f].cols; refs[f].h = frames[f].rows / 3 * 2; refs[f].stride = frames[f].step;
        }
        str_er_result *r = nullptr;
        check(str_er_detect_nv12_list(ctx_.get(), refs.data(), (int32_t)refs.size(), STR_ER_MEM_HOST, STR_ER_STAGE_ALL | STR_ER_WANT_NODES, &r));
        std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
        return unpack_batch(r, frames.size(), trees, root, pool, strong, weak);
    }

    // A list call's result (nf frames, STR_ER_WANT_NODES) as text_detect_batch hands it out -- also for the results of a str_er_stream
    // list submission.  Returns the result's 7-slot times vector.
    static std::vector<double> unpack_batch(const str_er_result *r, size_t nf, std::vector<std::vector<ERTree>> &trees, std::vector<ERs> &root,
                                            std::vector<std::vector<ERs>> &pool, std::vector<std::vector<ERs>> &strong,
                                            std::vector<std::vector<ERs>> &weak)
    {
        const int n = str_er_result_n_planes(r);
        std::vector<int> per(nf, 0), at(nf, 0);
        std::vector<str_er_plane_info> info((size_t)n);
        for (int i = 0; i < n; ++i) {
            str_er_result_plane_info(r, i, &info[(size_t)i]);
            if (info[(size_t)i].frame >= nf) throw std::runtime_error("unpack_batch: a plane of a frame beyond nf");
            ++per[info[(size_t)i].frame];
        }
        trees.assign(nf, std::vector<ERTree>()); root.assign(nf, ERs());
        pool.assign(nf, std::vector<ERs>()); strong.assign(nf, std::vector<ERs>()); weak.assign(nf, std::vector<ERs>());
        for (size_t f = 0; f < nf; ++f) {       // (sized first: the ERs point into the trees' node vectors)
            trees[f].assign((size_t)per[f], ERTree()); root[f].assign((size_t)per[f], nullptr);
            pool[f].assign((size_t)per[f], ERs()); strong[f].assign((size_t)per[f], ERs()); weak[f].assign((size_t)per[f], ERs());
        }
        for (int i = 0; i < n; ++i) {
            const size_t f = info[(size_t)i].frame, k = (size_t)at[f]++;
            unpack_plane(r, i, trees[f][k], pool[f][k], strong[f][k], weak[f][k]);
            root[f][k] = trees[f][k].root;
        }
        const double *t = str_er_result_times(r);
        return std::vector<double>(t, t + 7);
    }

    // ER* ERFilter::er_tree_extract(Mat input) (src/ER.cpp:240-374); input must be 8UC1 (:242)
    ER *er_tree_extract(const Image8 &input, ERTree &tree)
    {
        if (input.channels != 1) throw std::runtime_error("er_tree_extract: input.type() == CV_8UC1");
        str_er_result *r = nullptr;
        check(str_er_detect_planes(ctx_.get(), input.data, input.cols, input.rows, input.step, 0, 1, STR_ER_MEM_HOST,
                                   STR_ER_STAGE_EXTRACT | STR_ER_WANT_NODES, &r));
        std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
        ERs p, s, w;
        unpack_plane(r, 0, tree, p, s, w);
        return tree.root;
    }

    // void ERFilter::non_maximum_supression(ER *er, ERs &all, ERs &pool, Mat input) (src/ER.cpp:416-505);
    // `tree` is the table er_tree_extract filled.  pool comes back in ascending key order.
    void non_maximum_supression(ERTree &tree, ERs &all, ERs &pool, const Image8 &input, int *ambiguous = nullptr)
    {
        (void)all;
        std::vector<str_er_node> tab(tree.nodes.size());
        for (size_t i = 0; i < tab.size(); ++i) {
            const ER &e = tree.nodes[i];
            str_er_node &n = tab[i];
            n.key = e.key; n.parent = e.parent ? (int32_t)(e.parent - tree.nodes.data()) : (int32_t)i; n.area = e.area;
            n.x = (uint16_t)e.bound.x; n.y = (uint16_t)e.bound.y; n.w = (uint16_t)e.bound.width; n.h = (uint16_t)e.bound.height;
            n.level = (uint8_t)e.level; n.flags = (&e == tree.root) ? 1 : 0; n.reserved = 0;
            if (&e == tree.root) n.parent = (int32_t)i;
        }
        std::vector<int32_t> idx(tab.size());
        int32_t np = 0, amb = 0;
        // the table is in key order, so sibling ties are decided on the plane itself, by the reference's flood order
        if (input.data && input.channels == 1)
            check(str_er_nms_tree_plane(ctx_.get(), tab.data(), (int32_t)tab.size(), input.data, input.cols, input.rows, input.step,
                                        idx.data(), (int32_t)idx.size(), &np, &amb));
        else
            check(str_er_nms_tree(ctx_.get(), tab.data(), (int32_t)tab.size(), input.rows, input.cols, idx.data(),
                                  (int32_t)idx.size(), &np, &amb));
        pool.clear();
        for (int i = 0; i < np; ++i) pool.push_back(&tree.nodes[idx[i]]);
        if (ambiguous) *ambiguous = amb;
    }

    // void ERFilter::classify(ERs &pool, ERs &strong, ERs &weak, Mat input) (src/ER.cpp:507-528)
    void classify(ERs &pool, ERs &strong, ERs &weak, const Image8 &input)
    {
        const int n = (int)pool.size();
        std::vector<int32_t> boxes(4 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            boxes[4 * i] = pool[i]->bound.x; boxes[4 * i + 1] = pool[i]->bound.y;
            boxes[4 * i + 2] = pool[i]->bound.width; boxes[4 * i + 3] = pool[i]->bound.height;
        }
        std::vector<uint8_t> cls(n);
        std::vector<double> ss(n), sw(n);
        check(str_er_classify_boxes(ctx_.get(), input.data, input.cols, input.rows, input.step, boxes.data(), n, cls.data(),
                                    ss.data(), sw.data()));
        for (int i = 0; i < n; ++i) {
            pool[i]->score_strong = ss[i]; pool[i]->score_weak = sw[i];
            if (cls[i] == STR_ER_CLS_STRONG) strong.push_back(pool[i]);
            else if (cls[i] == STR_ER_CLS_WEAK) weak.push_back(pool[i]);
        }
    }

    // void ERFilter::compute_channels(Mat &src, Mat &YCrcb, vector<Mat> &channels) (src/ER.cpp:114-128):
    // six tightly packed planes [Y, Cr, Cb, 255-Y, 255-Cr, 255-Cb]
    void compute_channels(const Image8 &src, std::vector<std::vector<uint8_t>> &channels)
    {
        std::vector<uint8_t> six((size_t)6 * src.cols * src.rows);
        check(str_er_compute_channels(ctx_.get(), src.data, src.cols, src.rows, src.step, six.data()));
        const size_t n = (size_t)src.cols * src.rows;
        channels.assign(6, std::vector<uint8_t>());
        for (int i = 0; i < 6; ++i) channels[i].assign(six.begin() + i * n, six.begin() + (i + 1) * n);
    }

    // A recogniser-ready image of each line of `text` (str_er_line_crops): the line deskewed by its slope and resampled to the
    // context's crop height (set_line_crop), from the 8UC1 Y plane the lines were found on.  A line's boxes are its ERs' bounds as
    // er_grouping leaves them.  Crop t: geom (str_er_line_crop) and geom.height rows of geom.width bytes.
    struct LineCrop {
        str_er_line_crop geom{};
        std::vector<uint8_t> pixels;
    };
    void set_line_crop(int height = 32, int max_width = 1024, double pad = 0.125) { check(str_er_set_line_crop(ctx_.get(), height, max_width, pad)); }
    std::vector<LineCrop> text_crops(const Image8 &y_plane, const std::vector<Text> &text)
    {
        if (y_plane.channels != 1) throw std::runtime_error("text_crops expects an 8UC1 plane");
        std::vector<int32_t> boxes, first, count;
        std::vector<double>  slopes;
        for (const Text &t : text) {
            first.push_back((int32_t)(boxes.size() / 4));
            count.push_back((int32_t)t.ers.size());
            slopes.push_back(t.slope);
            for (const ER *e : t.ers) boxes.insert(boxes.end(), {e->bound.x, e->bound.y, e->bound.width, e->bound.height});
        }
        const int32_t n = (int32_t)text.size();
        std::vector<str_er_line_crop> recs(n ? n : 1);
        uint64_t n_bytes = 0;
        check(str_er_line_crops(ctx_.get(), y_plane.data, y_plane.cols, y_plane.rows, y_plane.step, boxes.data(), first.data(), count.data(),
                                slopes.data(), n, nullptr, 0, &n_bytes, recs.data()));
        std::vector<uint8_t> pix(n_bytes ? n_bytes : 1);
        if (n) check(str_er_line_crops(ctx_.get(), y_plane.data, y_plane.cols, y_plane.rows, y_plane.step, boxes.data(), first.data(), count.data(),
                                       slopes.data(), n, pix.data(), n_bytes, &n_bytes, recs.data()));
        std::vector<LineCrop> out((size_t)n);
        for (int32_t t = 0; t < n; ++t) {
            const str_er_line_crop &g = recs[(size_t)t];
            out[(size_t)t].geom = g;
            out[(size_t)t].pixels.assign(pix.begin() + (ptrdiff_t)g.pix_off, pix.begin() + (ptrdiff_t)(g.pix_off + (uint64_t)g.width * g.height));
        }
        return out;
    }

    // The pixels of ERs of one 8UC1 plane (str_er_er_masks): what the reference's flood visits for each ER and forgets.  Mask i is
    // ers[i]'s bound and, row by row over it, 1 for a pixel of the region (reachable from ER::key through 4-neighbours of level
    // <= ER::level inside the bound), 0 otherwise.  ER::key must be the canonical key of a region of this plane (as unpack_plane sets it).
    struct Mask {
        Rect bound;
        std::vector<uint8_t> pixels;     // bound.height rows of bound.width bytes
        int count = 0;                   // pixels set
    };
    std::vector<Mask> er_masks(const Image8 &plane, const ERs &ers)
    {
        if (plane.channels != 1) throw std::runtime_error("er_masks expects an 8UC1 plane");
        const std::vector<str_er_cand> regions = regions_of(ers);
        const int32_t n = (int32_t)regions.size();
        uint64_t      n_words = 0;
        check(str_er_er_masks(ctx_.get(), plane.data, plane.cols, plane.rows, plane.step, regions.data(), n, nullptr, 0, &n_words, nullptr));
        std::vector<uint32_t> bits(n_words ? n_words : 1);
        std::vector<uint32_t> count(n ? n : 1);
        if (n) check(str_er_er_masks(ctx_.get(), plane.data, plane.cols, plane.rows, plane.step, regions.data(), n, bits.data(), n_words, &n_words, count.data()));
        std::vector<Mask> out(ers.size());
        uint64_t off = 0;
        for (size_t i = 0; i < ers.size(); ++i) {
            const int w = regions[i].w, h = regions[i].h, pitch = (w + 31) / 32;
            Mask &m = out[i];
            m.bound = ers[i]->bound; m.count = (int)count[i];
            m.pixels.resize((size_t)w * h);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) m.pixels[(size_t)y * w + x] = (uint8_t)((bits[off + (size_t)y * pitch + (x >> 5)] >> (x & 31)) & 1u);
            off += (uint64_t)pitch * h;
        }
        return out;
    }

    // The descriptors of the same masks (str_er_er_shapes): perimeter, Euler number, hole pixels, crossings, convex-hull area and
    // grey moments, the features of cv::text::ERStat, as exact integers (include/str_er.h, str_er_shape).  The masks stay on the device.
    std::vector<str_er_shape> er_shapes(const Image8 &plane, const ERs &ers)
    {
        if (plane.channels != 1) throw std::runtime_error("er_shapes expects an 8UC1 plane");
        const std::vector<str_er_cand> regions = regions_of(ers);
        std::vector<str_er_shape> out(regions.size());
        check(str_er_er_shapes(ctx_.get(), plane.data, plane.cols, plane.rows, plane.step, regions.data(), (int32_t)regions.size(), out.data()));
        return out;
    }

    // The stroke-width descriptors of the same masks (str_er_er_strokes): the erosion depth K, the ridge and its depth moments, whose
    // mean gives the stroke width (include/str_er.h, str_er_stroke).  The masks stay on the device.
    std::vector<str_er_stroke> er_strokes(const Image8 &plane, const ERs &ers)
    {
        if (plane.channels != 1) throw std::runtime_error("er_strokes expects an 8UC1 plane");
        const std::vector<str_er_cand> regions = regions_of(ers);
        std::vector<str_er_stroke> out(regions.size());
        check(str_er_er_strokes(ctx_.get(), plane.data, plane.cols, plane.rows, plane.step, regions.data(), (int32_t)regions.size(), out.data()));
        return out;
    }

    // The text map of ERs of one 8UC1 plane (its level size) onto an out_w x out_h frame (str_er_text_map_regions): every frame pixel
    // the OR of values[i] over the ERs whose mask (that of er_masks) holds its sample (include/str_er.h, str_er_frame_map).  With ids
    // (one per ER, >= 0) also the smallest id covering each pixel, -1 where none does.  Both maps row-major, pitch out_w.
    struct FrameMap {
        int width = 0, height = 0;
        std::vector<uint8_t> text;          // STR_ER_TEXT_MAP_* bits
        std::vector<int32_t> line;          // line ids (empty without them)
    };
    FrameMap text_map_regions(const Image8 &plane, const ERs &ers, const std::vector<uint8_t> &values, int out_w, int out_h,
                              const std::vector<int32_t> *ids = nullptr)
    {
        if (plane.channels != 1) throw std::runtime_error("text_map_regions expects an 8UC1 plane");
        if (values.size() != ers.size() || (ids && ids->size() != ers.size())) throw std::runtime_error("text_map_regions: one value (and id) per ER");
        const std::vector<str_er_cand> regions = regions_of(ers);
        FrameMap m;
        m.width = out_w; m.height = out_h;
        m.text.resize((size_t)out_w * out_h);
        if (ids) m.line.resize((size_t)out_w * out_h);
        check(str_er_text_map_regions(ctx_.get(), plane.data, plane.cols, plane.rows, plane.step, regions.data(), values.data(),
                                      ids ? ids->data() : nullptr, (int32_t)regions.size(), out_w, out_h, m.text.data(), ids ? m.line.data() : nullptr));
        return m;
    }

    // The maps of every frame of a result of a call with STR_ER_WANT_TEXT_MAP and / or _LINE_MAP (str_er_result_frame_maps), copied out
    // of the result; a map whose flag was not given stays empty.
    static std::vector<FrameMap> frame_maps(const str_er_result *r)
    {
        int32_t  n = 0;
        uint64_t nb = 0, ni = 0;
        const str_er_frame_map *fm = str_er_result_frame_maps(r, &n);
        const uint8_t          *tm = str_er_result_text_map_pixels(r, &nb);
        const int32_t          *lm = str_er_result_line_map_ids(r, &ni);
        std::vector<FrameMap>   out(fm ? (size_t)n : 0);
        for (size_t f = 0; f < out.size(); ++f) {
            const size_t px = (size_t)fm[f].width * (size_t)fm[f].height;
            out[f].width = fm[f].width; out[f].height = fm[f].height;
            if (tm) out[f].text.assign(tm + fm[f].off, tm + fm[f].off + px);
            if (lm) out[f].line.assign(lm + fm[f].off, lm + fm[f].off + px);
        }
        return out;
    }

    // The text lines of every frame merged across pyramid levels (STR_ER_WANT_FRAME_LINES; the contract is at str_er_line_foot in
    // include/str_er.h): a foot per line of str_er_result_texts(), the pairs of lines with common pixels, the frame lines and the line
    // indices their first / count index.
    struct FrameLines {
        std::vector<str_er_line_foot>  feet;
        std::vector<str_er_line_pair>  pairs;
        std::vector<str_er_frame_line> lines;
        std::vector<int32_t>           members;
        std::vector<uint32_t>          bits;         // line_feet_regions only: the footprints, line after line (str_er_line_feet_regions)
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static FrameLines frame_lines(const str_er_result *r)
    {
        FrameLines out;
        int32_t n = 0;
        if (const str_er_line_foot *p = str_er_result_line_feet(r, &n)) out.feet.assign(p, p + n);
        if (const str_er_line_pair *p = str_er_result_line_pairs(r, &n)) out.pairs.assign(p, p + n);
        if (const str_er_frame_line *p = str_er_result_frame_lines(r, &n)) out.lines.assign(p, p + n);
        if (const int32_t *p = str_er_result_frame_line_members(r, &n)) out.members.assign(p, p + n);
        return out;
    }
    // two lines of a frame are duplicates from a Jaccard index of num / den of their footprints on (str_er_set_frame_merge)
    void set_frame_merge(int num, int den) { check(str_er_set_frame_merge(ctx_.get(), num, den)); }
    // The footprints and overlaps of n_lines lines made of ERs of one 8UC1 plane (ER i belongs to line line_of[i]) on an out_w x out_h
    // frame (str_er_line_feet_regions); the frame lines of the one frame by str_er_frame_lines_from_pairs at the context's threshold
    FrameLines line_feet_regions(const Image8 &plane, const ERs &ers, const std::vector<int32_t> &line_of, int n_lines, int out_w, int out_h)
    {
        if (plane.channels != 1) throw std::runtime_error("line_feet_regions expects an 8UC1 plane");
        if (line_of.size() != ers.size() || n_lines < 0) throw std::runtime_error("line_feet_regions: one line per ER");
        const std::vector<str_er_cand> regions = regions_of(ers);
        FrameLines out;
        out.feet.resize((size_t)n_lines);
        uint64_t n_words = 0;
        int32_t  n_pairs = 0;
        check(str_er_line_feet_regions(ctx_.get(), plane.data, plane.cols, plane.rows, plane.step, regions.data(), line_of.data(), (int32_t)regions.size(),
                                       n_lines, out_w, out_h, out.feet.data(), nullptr, 0, &n_words, nullptr, 0, &n_pairs));
        out.bits.resize((size_t)n_words);
        out.pairs.resize((size_t)n_pairs);
        check(str_er_line_feet_regions(ctx_.get(), plane.data, plane.cols, plane.rows, plane.step, regions.data(), line_of.data(), (int32_t)regions.size(),
                                       n_lines, out_w, out_h, out.feet.data(), out.bits.empty() ? nullptr : out.bits.data(), n_words, &n_words,
                                       out.pairs.empty() ? nullptr : out.pairs.data(), n_pairs, &n_pairs));
        return out;
    }

    // The convex hull, the moments and the oriented box of every text line and of every frame line (STR_ER_WANT_LINE_GEOM; the contract is
    // at str_er_line_geom in include/str_er.h): one record per line of str_er_result_texts(), one per frame line, and the vertices
    // (x, y pairs) that the first / count of both index.
    struct LineGeoms {
        std::vector<str_er_line_geom> lines, frame_lines;
        std::vector<int32_t>          points;
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static LineGeoms line_geoms(const str_er_result *r)
    {
        LineGeoms out;
        int32_t n = 0;
        if (const str_er_line_geom *p = str_er_result_line_geoms(r, &n)) out.lines.assign(p, p + n);
        if (const str_er_line_geom *p = str_er_result_frame_line_geoms(r, &n)) out.frame_lines.assign(p, p + n);
        if (const int32_t *p = str_er_result_geom_points(r, &n)) out.points.assign(p, p + 2 * (size_t)n);
        return out;
    }
    // the geometry of footprints of one frame size on the GPU (str_er_feet_geom): feet and bits as str_er_link_feet takes them
    LineGeoms feet_geom(int32_t width, int32_t height, const std::vector<str_er_line_foot> &feet, const std::vector<uint32_t> &bits)
    {
        LineGeoms out;
        out.lines.resize(feet.size());
        int64_t cap = 1;                                  // (a hull has at most two vertices per height 0 .. h: one call)
        for (const str_er_line_foot &f : feet) cap += 2 * ((int64_t)(f.h > 0 ? f.h : 0) + 1);
        if (cap > INT32_MAX) cap = INT32_MAX;
        out.points.resize(2 * (size_t)cap);
        int32_t n = 0;
        check(str_er_feet_geom(ctx_.get(), width, height, feet.empty() ? nullptr : feet.data(), bits.empty() ? nullptr : bits.data(), (int32_t)feet.size(),
                               out.lines.empty() ? nullptr : out.lines.data(), out.points.data(), (int32_t)cap, &n));
        out.points.resize(2 * (size_t)n);
        return out;
    }

    // Every text line split into glyph runs and words (STR_ER_WANT_LINE_WORDS; the contract is at str_er_line_run in include/str_er.h): one
    // record per line of str_er_result_texts(), and the runs and words they index.  A frame line's words are those of its rep.
    struct LineWords {
        std::vector<str_er_line_words> lines;
        std::vector<str_er_line_run>   runs;
        std::vector<str_er_line_word>  words;
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static LineWords line_words(const str_er_result *r)
    {
        LineWords out;
        int32_t n = 0;
        if (const str_er_line_words *p = str_er_result_line_words(r, &n)) out.lines.assign(p, p + n);
        if (const str_er_line_run *p = str_er_result_line_runs(r, &n)) out.runs.assign(p, p + n);
        if (const str_er_line_word *p = str_er_result_words(r, &n)) out.words.assign(p, p + n);
        return out;
    }
    // the gap that breaks a word: gap * den >= num * colmax (str_er_set_word_gap; 1 / 3 by default)
    void set_word_gap(int32_t num, int32_t den) { check(str_er_set_word_gap(ctx_.get(), num, den)); }
    // the runs and words of footprints of one frame size, the runs made on the GPU (str_er_feet_words): feet and bits as feet_geom takes them
    LineWords feet_words(int32_t width, int32_t height, const std::vector<str_er_line_foot> &feet, const std::vector<uint32_t> &bits)
    {
        LineWords out;
        out.lines.resize(feet.size());
        int64_t cap = 1;                                  // (a row of w columns holds at most (w + 1) / 2 runs: one call)
        for (const str_er_line_foot &f : feet) cap += ((int64_t)(f.w > 0 ? f.w : 0) + 1) / 2;
        if (cap > INT32_MAX) cap = INT32_MAX;
        out.runs.resize((size_t)cap);
        out.words.resize((size_t)cap);
        int32_t nr = 0, nw = 0;
        check(str_er_feet_words(ctx_.get(), width, height, feet.empty() ? nullptr : feet.data(), bits.empty() ? nullptr : bits.data(), (int32_t)feet.size(),
                                out.lines.empty() ? nullptr : out.lines.data(), out.runs.data(), (int32_t)cap, &nr, out.words.data(), (int32_t)cap, &nw));
        out.runs.resize((size_t)nr);
        out.words.resize((size_t)nw);
        return out;
    }

    // Every glyph run read by the OCR scorer (STR_ER_WANT_RUN_READ; the contract is at str_er_run_read in include/str_er.h): one record per
    // run of LineWords::runs, in the same order, and 1800 feature bytes per run.  Needs an SVM model of dim 1800 in the context.
    struct RunReads {
        std::vector<str_er_run_read> reads;
        std::vector<uint8_t>         features;
    };
    // ... copied out of the result of a call with the flag (both empty without it)
    static RunReads run_reads(const str_er_result *r)
    {
        RunReads out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_run_read *p = str_er_result_run_reads(r, &n)) out.reads.assign(p, p + n);
        if (const uint8_t *p = str_er_result_run_features(r, &nb)) out.features.assign(p, p + nb);
        return out;
    }
    // the string of word w: the characters of its runs
    static std::string word_text(const LineWords &lw, const RunReads &rd, size_t w)
    {
        std::string s;
        const str_er_line_word &W = lw.words.at(w);
        for (int32_t k = W.first_run; k < W.first_run + W.n_runs; ++k) s.push_back((char)rd.reads.at((size_t)k).ch);
        return s;
    }
    // the text of line t: its words joined by one blank (a frame line's text is that of its rep)
    static std::string line_text(const LineWords &lw, const RunReads &rd, size_t t)
    {
        std::string s;
        const str_er_line_words &L = lw.lines.at(t);
        for (int32_t k = L.first_word; k < L.first_word + L.n_words; ++k) s += (k > L.first_word ? " " : "") + word_text(lw, rd, (size_t)k);
        return s;
    }
    // feet_words and the reading of every run (str_er_feet_read): slopes one per foot, or empty: all 0; want_reads = false: the features
    // only (no model needed)
    std::pair<LineWords, RunReads> feet_read(int32_t width, int32_t height, const std::vector<str_er_line_foot> &feet, const std::vector<uint32_t> &bits,
                                             const std::vector<double> &slopes = {}, bool want_reads = true)
    {
        if (!slopes.empty() && slopes.size() != feet.size()) throw std::invalid_argument("feet_read: one slope per foot");
        LineWords lw;
        RunReads  rd;
        lw.lines.resize(feet.size());
        const str_er_line_foot *fp = feet.empty() ? nullptr : feet.data();
        const uint32_t         *bp = bits.empty() ? nullptr : bits.data();
        const double           *sp = slopes.empty() ? nullptr : slopes.data();
        str_er_line_words      *lp = lw.lines.empty() ? nullptr : lw.lines.data();
        int32_t nr = 0, nw = 0;
        check(str_er_feet_read(ctx_.get(), width, height, fp, bp, sp, (int32_t)feet.size(), lp, nullptr, 0, &nr, nullptr, 0, &nw, nullptr, nullptr));      // (counts)
        lw.runs.resize((size_t)nr + 1);
        lw.words.resize((size_t)nw + 1);
        rd.reads.resize(want_reads ? (size_t)nr + 1 : 0);
        rd.features.resize(1800 * ((size_t)nr + 1));
        check(str_er_feet_read(ctx_.get(), width, height, fp, bp, sp, (int32_t)feet.size(), lp, lw.runs.data(), nr + 1, &nr, lw.words.data(), nw + 1, &nw,
                               want_reads ? rd.reads.data() : nullptr, rd.features.data()));
        lw.runs.resize((size_t)nr);
        lw.words.resize((size_t)nw);
        if (want_reads) rd.reads.resize((size_t)nr);
        rd.features.resize(1800 * (size_t)nr);
        return {std::move(lw), std::move(rd)};
    }

    // Every word matched against a lexicon (STR_ER_WANT_WORD_MATCH; the contract is at str_er_word_match in include/str_er.h): one record
    // per word of LineWords::words, the 65 cost bytes of every run and its class probabilities (probs.size() / n runs a run).  Needs
    // STR_ER_WANT_RUN_READ and a lexicon in the context.
    struct WordMatches {
        std::vector<str_er_word_match> matches;
        std::vector<uint8_t>           costs;
        std::vector<double>            probs;
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static WordMatches word_matches(const str_er_result *r)
    {
        WordMatches out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_word_match *p = str_er_result_word_matches(r, &n)) out.matches.assign(p, p + n);
        if (const uint8_t *p = str_er_result_run_costs(r, &nb)) out.costs.assign(p, p + nb);
        if (const double *p = str_er_result_run_probs(r, &nb)) out.probs.assign(p, p + nb);
        return out;
    }
    // the lexicon of the matcher: words of 1 .. 32 characters of the alphabet of str_er_ocr_char, at most 2^20; none clears it
    void set_lexicon(const std::vector<std::string> &words, bool fold_case = true)
    {
        std::string          bytes;
        std::vector<int32_t> offsets{0};
        for (const std::string &w : words) {
            bytes += w;
            if (bytes.size() > (size_t)INT32_MAX) throw std::invalid_argument("set_lexicon: too many bytes");
            offsets.push_back((int32_t)bytes.size());
        }
        check(str_er_set_lexicon(ctx_.get(), bytes.data(), offsets.data(), (int32_t)words.size(), fold_case ? STR_ER_LEXICON_FOLD_CASE : 0u));
    }
    // INS, DEL (1 .. 255) and the band (0 .. 31) of the matcher (str_er_set_word_match; 64, 64, 2 by default)
    void set_word_match(int32_t ins, int32_t del, int32_t band) { check(str_er_set_word_match(ctx_.get(), ins, del, band)); }
    // the cost rows (65 bytes a run) of n x nr_class class probabilities, with the labels of the loaded model (str_er_run_costs)
    std::vector<uint8_t> run_costs(const std::vector<double> &prob, int32_t n)
    {
        std::vector<uint8_t> out(65 * (size_t)(n > 0 ? n : 0));
        check(str_er_run_costs(ctx_.get(), prob.empty() ? nullptr : prob.data(), n, out.empty() ? nullptr : out.data()));
        return out;
    }
    // the words [first_run[w], first_run[w] + n_runs[w]) of the caller's cost rows against the lexicon (str_er_match_words)
    std::vector<str_er_word_match> match_words(const std::vector<uint8_t> &costs, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs)
    {
        if (first_run.size() != n_runs.size() || costs.size() % 65) throw std::invalid_argument("match_words: 65 bytes a run, one span a word");
        std::vector<str_er_word_match> out(first_run.size());
        check(str_er_match_words(ctx_.get(), costs.empty() ? nullptr : costs.data(), (int32_t)(costs.size() / 65), first_run.empty() ? nullptr : first_run.data(),
                                 n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(), out.empty() ? nullptr : out.data()));
        return out;
    }
    // the matched string of word w: the lexicon entry (as given in `lexicon`) that matches it best, its own reading where none does
    static std::string word_match_text(const LineWords &lw, const RunReads &rd, const WordMatches &wm, const std::vector<std::string> &lexicon, size_t w)
    {
        const int32_t e = wm.matches.at(w).entry;
        return e >= 0 && (size_t)e < lexicon.size() ? lexicon[(size_t)e] : word_text(lw, rd, w);
    }
    // the matched text of line t: its words' matched strings joined by one blank
    static std::string line_match_text(const LineWords &lw, const RunReads &rd, const WordMatches &wm, const std::vector<std::string> &lexicon, size_t t)
    {
        std::string s;
        const str_er_line_words &L = lw.lines.at(t);
        for (int32_t k = L.first_word; k < L.first_word + L.n_words; ++k) s += (k > L.first_word ? " " : "") + word_match_text(lw, rd, wm, lexicon, (size_t)k);
        return s;
    }

    // The words of adjacent frames linked into word tracks and one lexicon match per word track over the cost rows of all its members
    // (STR_ER_WANT_TRACK_READ; the contract is at str_er_word_link in include/str_er.h): the links, the tracks, the word indices their
    // first / count index, the track of every word (-1: not eligible), one match per track and one cost per slot of the member array.
    // Needs STR_ER_WANT_LINE_LINKS and STR_ER_WANT_WORD_MATCH.
    struct TrackRead {
        std::vector<str_er_word_link>   links;
        std::vector<str_er_word_track>  tracks;
        std::vector<int32_t>            members, track_of_words;
        std::vector<str_er_track_match> matches;
        std::vector<int32_t>            member_costs;
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static TrackRead track_read(const str_er_result *r)
    {
        TrackRead out;
        int32_t n = 0;
        if (const str_er_word_link *p = str_er_result_word_links(r, &n)) out.links.assign(p, p + n);
        if (const str_er_word_track *p = str_er_result_word_tracks(r, &n)) out.tracks.assign(p, p + n);
        if (const int32_t *p = str_er_result_word_track_members(r, &n)) out.members.assign(p, p + n);
        if (const int32_t *p = str_er_result_word_track_of_words(r, &n)) out.track_of_words.assign(p, p + n);
        if (const str_er_track_match *p = str_er_result_track_matches(r, &n)) out.matches.assign(p, p + n);
        if (const int32_t *p = str_er_result_track_member_costs(r, &n)) out.member_costs.assign(p, p + n);
        return out;
    }
    // two words of adjacent frames are linked from a Jaccard index of num / den of their boxes on (str_er_set_word_link)
    void set_word_link(int num, int den) { check(str_er_set_word_link(ctx_.get(), num, den)); }
    // the tracks members[track_first[g] .. track_first[g] + track_count[g]) of the words of the caller's cost rows against the lexicon
    // (str_er_match_tracks): the records, and in member_cost one cost per slot of members
    std::vector<str_er_track_match> match_tracks(const std::vector<uint8_t> &costs, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs,
                                                 const std::vector<int32_t> &track_first, const std::vector<int32_t> &track_count,
                                                 const std::vector<int32_t> &members, std::vector<int32_t> &member_cost)
    {
        if (first_run.size() != n_runs.size() || track_first.size() != track_count.size() || costs.size() % 65)
            throw std::invalid_argument("match_tracks: 65 bytes a run, one span a word, one span a track");
        std::vector<str_er_track_match> out(track_first.size());
        member_cost.assign(members.size(), -1);
        check(str_er_match_tracks(ctx_.get(), costs.empty() ? nullptr : costs.data(), (int32_t)(costs.size() / 65), first_run.empty() ? nullptr : first_run.data(),
                                  n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(), track_first.empty() ? nullptr : track_first.data(),
                                  track_count.empty() ? nullptr : track_count.data(), members.empty() ? nullptr : members.data(), (int32_t)members.size(),
                                  (int32_t)track_first.size(), out.empty() ? nullptr : out.data(), member_cost.empty() ? nullptr : member_cost.data()));
        return out;
    }
    // the string of word track g: the lexicon entry it takes (as given in `lexicon`), its representative's own reading where it has none
    static std::string word_track_text(const LineWords &lw, const RunReads &rd, const TrackRead &tr, const std::vector<std::string> &lexicon, size_t g)
    {
        const int32_t e = tr.matches.at(g).entry;
        return e >= 0 && (size_t)e < lexicon.size() ? lexicon[(size_t)e] : word_text(lw, rd, (size_t)tr.tracks.at(g).rep);
    }

    // Every word track decoded without a lexicon: the median string of its members under the bigram table, from the members' own decoder
    // strings by single edits (STR_ER_WANT_TRACK_DECODE; the contract is at str_er_track_decode in include/str_er.h): one record and 32
    // label bytes per word track (0xFF past n_chars), one cost per slot of the member array.  The links and tracks come with the flag:
    // track_read(r) fills them (its matches stay empty without STR_ER_WANT_TRACK_READ).  Needs STR_ER_WANT_LINE_LINKS, STR_ER_WANT_WORD_DECODE
    // and a table in the context; no lexicon.
    struct TrackDecodes {
        std::vector<str_er_track_decode> decodes;
        std::vector<uint8_t>             chars;
        std::vector<int32_t>             member_costs;
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static TrackDecodes track_decodes(const str_er_result *r)
    {
        TrackDecodes out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_track_decode *p = str_er_result_track_decodes(r, &n)) out.decodes.assign(p, p + n);
        if (const uint8_t *p = str_er_result_track_decode_chars(r, &nb)) out.chars.assign(p, p + nb);
        if (const int32_t *p = str_er_result_track_decode_member_costs(r, &n)) out.member_costs.assign(p, p + n);
        return out;
    }
    // INS and DEL (1 .. 255) and the polish rounds (0 .. 64) of the track decode (str_er_set_track_decode; 64, 64 and 8 by default)
    void set_track_decode(int32_t ins, int32_t del, int32_t rounds) { check(str_er_set_track_decode(ctx_.get(), ins, del, rounds)); }
    // the tracks members[track_first[g] .. track_first[g] + track_count[g]) of the words of the caller's cost rows under the table
    // (str_er_decode_tracks)
    TrackDecodes decode_tracks(const std::vector<uint8_t> &costs, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs,
                               const std::vector<int32_t> &track_first, const std::vector<int32_t> &track_count, const std::vector<int32_t> &members)
    {
        if (first_run.size() != n_runs.size() || track_first.size() != track_count.size() || costs.size() % 65)
            throw std::invalid_argument("decode_tracks: 65 bytes a run, one span a word, one span a track");
        TrackDecodes out;
        out.decodes.resize(track_first.size());
        out.chars.resize(32 * track_first.size());
        out.member_costs.assign(members.size(), -1);
        check(str_er_decode_tracks(ctx_.get(), costs.empty() ? nullptr : costs.data(), (int32_t)(costs.size() / 65), first_run.empty() ? nullptr : first_run.data(),
                                   n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(), track_first.empty() ? nullptr : track_first.data(),
                                   track_count.empty() ? nullptr : track_count.data(), members.empty() ? nullptr : members.data(), (int32_t)members.size(),
                                   (int32_t)track_first.size(), out.decodes.empty() ? nullptr : out.decodes.data(), out.chars.empty() ? nullptr : out.chars.data(),
                                   out.member_costs.empty() ? nullptr : out.member_costs.data()));
        return out;
    }
    // the string word track g was decoded to: its representative's own reading where the track was not decoded (no seed)
    static std::string word_track_decode_text(const LineWords &lw, const RunReads &rd, const TrackRead &tr, const TrackDecodes &td, size_t g)
    {
        const str_er_track_decode &d = td.decodes.at(g);
        if (d.cost < 0) return word_text(lw, rd, (size_t)tr.tracks.at(g).rep);
        std::string s;
        for (int32_t k = 0; k < d.n_chars; ++k) s += (char)str_er_ocr_char(td.chars.at(32 * g + (size_t)k));
        return s;
    }

    // Every word decoded under a character bigram table (STR_ER_WANT_WORD_DECODE; the contract is at str_er_word_decode in
    // include/str_er.h): one record per word of LineWords::words, 64 label bytes and 64 source bytes per word (0xFF past n_chars), and
    // the cost bytes and class probabilities of the runs as in WordMatches.  Needs STR_ER_WANT_RUN_READ and a table in the context.
    struct WordDecodes {
        std::vector<str_er_word_decode> decodes;
        std::vector<uint8_t>            chars, src;
        std::vector<uint8_t>            costs;
        std::vector<double>             probs;
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static WordDecodes word_decodes(const str_er_result *r)
    {
        WordDecodes out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_word_decode *p = str_er_result_word_decodes(r, &n)) out.decodes.assign(p, p + n);
        if (const uint8_t *p = str_er_result_word_decode_chars(r, &nb)) out.chars.assign(p, p + nb);
        if (const uint8_t *p = str_er_result_word_decode_src(r, &nb)) out.src.assign(p, p + nb);
        if (const uint8_t *p = str_er_result_run_costs(r, &nb)) out.costs.assign(p, p + nb);
        if (const double *p = str_er_result_run_probs(r, &nb)) out.probs.assign(p, p + nb);
        return out;
    }
    // the table of the decoder: 66 x 66 cost bytes (str_er_set_bigram); an empty vector removes it
    void set_bigram(const std::vector<uint8_t> &table)
    {
        if (!table.empty() && table.size() != 66 * 66) throw std::invalid_argument("set_bigram: 66 x 66 bytes");
        check(str_er_set_bigram(ctx_.get(), table.empty() ? nullptr : table.data()));
    }
    // a table from 65 x 65 probabilities P(b after a) and, optionally, 65 of beginning with and 65 of ending on a character
    static std::vector<uint8_t> bigram_from_probs(const std::vector<double> &tp, const std::vector<double> &start = {}, const std::vector<double> &end = {})
    {
        if (tp.size() != 65 * 65 || (!start.empty() && start.size() != 65) || (!end.empty() && end.size() != 65))
            throw std::invalid_argument("bigram_from_probs: 65 x 65 probabilities, 65 start and 65 end values");
        std::vector<uint8_t> out(66 * 66);
        if (str_er_bigram_from_probs(tp.data(), start.empty() ? nullptr : start.data(), end.empty() ? nullptr : end.data(), out.data()) != STR_ER_OK)
            throw std::invalid_argument("bigram_from_probs");
        return out;
    }
    // INS and DEL (0 .. 255, 0: off) of the decoder (str_er_set_word_decode; 0, 0 by default)
    void set_word_decode(int32_t ins, int32_t del) { check(str_er_set_word_decode(ctx_.get(), ins, del)); }
    // the words [first_run[w], first_run[w] + n_runs[w]) of the caller's cost rows under the table (str_er_decode_words)
    WordDecodes decode_words(const std::vector<uint8_t> &costs, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs)
    {
        if (first_run.size() != n_runs.size() || costs.size() % 65) throw std::invalid_argument("decode_words: 65 bytes a run, one span a word");
        WordDecodes out;
        out.decodes.resize(first_run.size());
        out.chars.resize(64 * first_run.size());
        out.src.resize(64 * first_run.size());
        check(str_er_decode_words(ctx_.get(), costs.empty() ? nullptr : costs.data(), (int32_t)(costs.size() / 65), first_run.empty() ? nullptr : first_run.data(),
                                  n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(), out.decodes.empty() ? nullptr : out.decodes.data(),
                                  out.chars.empty() ? nullptr : out.chars.data(), out.src.empty() ? nullptr : out.src.data()));
        return out;
    }
    // The margins of the decoded words (str_er_set_word_margin beside STR_ER_WANT_WORD_DECODE; the contract is at str_er_word_margin in
    // include/str_er.h): one record per word, and per word 32 row margins (-1 past its rows), 32 row readings and 32 row alternatives
    // (0xFF past its rows; 65: the row dropped); marginals only from word_margins on the caller's rows, 32 x 66 per word
    struct WordMargins {
        std::vector<str_er_word_margin> margins;
        std::vector<int32_t>            row_margins, marginals;
        std::vector<uint8_t>            row_reads, row_alts;
    };
    // whether a call with STR_ER_WANT_WORD_DECODE also makes the margins (str_er_set_word_margin; off by default)
    void set_word_margin(bool on) { check(str_er_set_word_margin(ctx_.get(), on ? 1 : 0)); }
    // ... copied out of the result of such a call (all empty when it made none)
    static WordMargins word_margins(const str_er_result *r)
    {
        WordMargins out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_word_margin *p = str_er_result_word_margins(r, &n)) out.margins.assign(p, p + n);
        if (const int32_t *p = str_er_result_word_row_margins(r, &nb)) out.row_margins.assign(p, p + nb / 4);
        if (const uint8_t *p = str_er_result_word_row_reads(r, &nb)) out.row_reads.assign(p, p + nb);
        if (const uint8_t *p = str_er_result_word_row_alts(r, &nb)) out.row_alts.assign(p, p + nb);
        return out;
    }
    // the margins of the words [first_run[w], first_run[w] + n_runs[w]) of the caller's cost rows under the table (str_er_word_margins)
    WordMargins word_margins(const std::vector<uint8_t> &costs, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs, bool marginals = false)
    {
        if (first_run.size() != n_runs.size() || costs.size() % 65) throw std::invalid_argument("word_margins: 65 bytes a run, one span a word");
        const size_t n = first_run.size();
        WordMargins  out;
        out.margins.resize(n);
        out.row_margins.resize(32 * n);
        out.row_reads.resize(32 * n);
        out.row_alts.resize(32 * n);
        if (marginals) out.marginals.resize(32 * 66 * n);
        check(str_er_word_margins(ctx_.get(), costs.empty() ? nullptr : costs.data(), (int32_t)(costs.size() / 65), n ? first_run.data() : nullptr,
                                  n ? n_runs.data() : nullptr, (int32_t)n, n ? out.margins.data() : nullptr, n ? out.row_margins.data() : nullptr,
                                  n ? out.row_reads.data() : nullptr, n ? out.row_alts.data() : nullptr, marginals && n ? out.marginals.data() : nullptr));
        return out;
    }
    // The margins of the decoded lines (str_er_set_line_margin beside str_er_set_line_decode and STR_ER_WANT_WORD_DECODE; the contract is at
    // str_er_line_margin in include/str_er.h): one record per line, and per row of the line decode's rows a row margin and a gap margin
    // (-1 where there is none), a reading, an alternative (65: the row dropped) and a gap move (0 join, 1 break; 0xFF where there is
    // none); marginals only from line_margins on the caller's rows, 68 per row
    struct LineMargins {
        std::vector<str_er_line_margin> margins;
        std::vector<int32_t>            row_margins, gap_margins, marginals;
        std::vector<uint8_t>            row_reads, row_alts, gap_moves;
    };
    // whether a call that decodes its lines also makes their margins (str_er_set_line_margin; off by default)
    void set_line_margin(bool on) { check(str_er_set_line_margin(ctx_.get(), on ? 1 : 0)); }
    // ... copied out of the result of such a call (all empty when it made none)
    static LineMargins line_margins(const str_er_result *r)
    {
        LineMargins out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_line_margin *p = str_er_result_line_margins(r, &n)) out.margins.assign(p, p + n);
        if (const int32_t *p = str_er_result_line_row_margins(r, &nb)) out.row_margins.assign(p, p + nb / 4);
        if (const uint8_t *p = str_er_result_line_row_reads(r, &nb)) out.row_reads.assign(p, p + nb);
        if (const uint8_t *p = str_er_result_line_row_alts(r, &nb)) out.row_alts.assign(p, p + nb);
        if (const int32_t *p = str_er_result_line_gap_margins(r, &nb)) out.gap_margins.assign(p, p + nb / 4);
        if (const uint8_t *p = str_er_result_line_gap_moves(r, &nb)) out.gap_moves.assign(p, p + nb);
        return out;
    }
    // the margins of the lines [first_row[t], first_row[t] + n_rows[t]) of the caller's cost rows and gap pairs under the table
    // (str_er_line_margins: the line decoder and its margins in one call)
    LineMargins line_margins(const std::vector<uint8_t> &costs, const std::vector<uint8_t> &gaps, const std::vector<int32_t> &first_row, const std::vector<int32_t> &n_rows,
                             bool marginals = false)
    {
        if (first_row.size() != n_rows.size() || costs.size() % 65 || gaps.size() != 2 * (costs.size() / 65))
            throw std::invalid_argument("line_margins: 65 bytes and one gap pair a row, one span a line");
        const size_t n = first_row.size(), nr = costs.size() / 65;
        LineMargins  out;
        out.margins.resize(n);
        out.row_margins.resize(nr); out.gap_margins.resize(nr);
        out.row_reads.resize(nr); out.row_alts.resize(nr); out.gap_moves.resize(nr);
        if (marginals) out.marginals.resize(68 * nr);
        check(str_er_line_margins(ctx_.get(), nr ? costs.data() : nullptr, (int32_t)nr, nr ? gaps.data() : nullptr, n ? first_row.data() : nullptr, n ? n_rows.data() : nullptr,
                                  (int32_t)n, n ? out.margins.data() : nullptr, nr ? out.row_margins.data() : nullptr, nr ? out.row_reads.data() : nullptr,
                                  nr ? out.row_alts.data() : nullptr, nr ? out.gap_margins.data() : nullptr, nr ? out.gap_moves.data() : nullptr,
                                  marginals && nr ? out.marginals.data() : nullptr));
        return out;
    }
    // the decoded string of word w: its own reading where it was not decoded (more than 32 runs)
    static std::string word_decode_text(const LineWords &lw, const RunReads &rd, const WordDecodes &wd, size_t w)
    {
        const str_er_word_decode &d = wd.decodes.at(w);
        if (d.cost < 0) return word_text(lw, rd, w);
        std::string s;
        for (int32_t k = 0; k < d.n_chars; ++k) s += (char)str_er_ocr_char(wd.chars.at(64 * w + (size_t)k));
        return s;
    }
    // per character of word_decode_text(w): the index of the run it came from in LineWords::runs, and whether it was inserted behind it
    static std::vector<std::pair<int32_t, bool>> word_decode_runs(const LineWords &lw, const WordDecodes &wd, size_t w)
    {
        std::vector<std::pair<int32_t, bool>> out;
        const str_er_word_decode &d = wd.decodes.at(w);
        const str_er_line_word   &W = lw.words.at(w);
        if (d.cost < 0)
            for (int32_t k = 0; k < W.n_runs; ++k) out.emplace_back(W.first_run + k, false);
        else
            for (int32_t k = 0; k < d.n_chars; ++k) {
                const uint8_t v = wd.src.at(64 * w + (size_t)k);
                out.emplace_back(W.first_run + (v & 0x7F), (v & 0x80) != 0);
            }
        return out;
    }
    // the decoded text of line t: its words' decoded strings joined by one blank
    static std::string line_decode_text(const LineWords &lw, const RunReads &rd, const WordDecodes &wd, size_t t)
    {
        std::string s;
        const str_er_line_words &L = lw.lines.at(t);
        for (int32_t k = L.first_word; k < L.first_word + L.n_words; ++k) s += (k > L.first_word ? " " : "") + word_decode_text(lw, rd, wd, (size_t)k);
        return s;
    }

    // Touching glyphs split (STR_ER_WANT_RUN_SPLIT; the contract is at str_er_run_split in include/str_er.h): one split record per run of
    // LineWords::runs, the pieces they index with one reading and 65 cost bytes each, the parts of the words back to back in word order
    // (piece -1: the whole run), one record per word of LineWords::words, and the 65 cost bytes of every run.  Needs STR_ER_WANT_RUN_READ.
    struct RunSplits {
        std::vector<str_er_run_split>  splits;
        std::vector<str_er_run_piece>  pieces;
        std::vector<str_er_run_read>   piece_reads;
        std::vector<uint8_t>           piece_costs, piece_features;      // (the features: feet_split alone)
        std::vector<str_er_split_part> parts;
        std::vector<str_er_word_split> word_splits;
        std::vector<uint8_t>           run_costs;
        std::vector<uint8_t>           part_costs;                       // (the parts' rows: split_words alone)
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static RunSplits run_splits(const str_er_result *r)
    {
        RunSplits out;
        int32_t   n = 0;
        uint64_t  nb = 0;
        if (const str_er_run_split *p = str_er_result_run_splits(r, &n)) out.splits.assign(p, p + n);
        if (const str_er_run_piece *p = str_er_result_run_pieces(r, &n)) out.pieces.assign(p, p + n);
        if (const str_er_run_read *p = str_er_result_piece_reads(r, &n)) out.piece_reads.assign(p, p + n);
        if (const uint8_t *p = str_er_result_piece_costs(r, &nb)) out.piece_costs.assign(p, p + nb);
        if (const str_er_split_part *p = str_er_result_split_parts(r, &n)) out.parts.assign(p, p + n);
        if (const str_er_word_split *p = str_er_result_word_splits(r, &n)) out.word_splits.assign(p, p + n);
        if (str_er_result_run_splits(r, &n))          // (the runs' rows come with other flags too: here only with this one)
            if (const uint8_t *p = str_er_result_run_costs(r, &nb)) out.run_costs.assign(p, p + nb);
        return out;
    }
    // the valley threshold num / den of a run's height (1 .. 65535 each) and SPLIT (0 .. 255) (str_er_set_run_split; 1 / 4 and 8 by default)
    void set_run_split(int32_t num, int32_t den, int32_t split_cost) { check(str_er_set_run_split(ctx_.get(), num, den, split_cost)); }
    // the kept cut columns of one run from its column counts and height, relative to the run (str_er_cuts_from_counts; pure host)
    static std::vector<int32_t> cuts_from_counts(const std::vector<uint32_t> &counts, int32_t height, int32_t num = 1, int32_t den = 4)
    {
        int32_t cut[3], n = 0;
        if (str_er_cuts_from_counts(counts.empty() ? nullptr : counts.data(), (int32_t)counts.size(), height, num, den, cut, &n, nullptr) != STR_ER_OK)
            throw std::invalid_argument("cuts_from_counts");
        return std::vector<int32_t>(cut, cut + n);
    }
    // feet_read and the cuts and pieces of every run, the pieces read with the runs (str_er_feet_split): slopes one per foot, or empty:
    // all 0; want_reads = false: cuts, pieces and features only (no model needed)
    std::tuple<LineWords, RunReads, RunSplits> feet_split(int32_t width, int32_t height, const std::vector<str_er_line_foot> &feet,
                                                          const std::vector<uint32_t> &bits, const std::vector<double> &slopes = {}, bool want_reads = true)
    {
        if (!slopes.empty() && slopes.size() != feet.size()) throw std::invalid_argument("feet_split: one slope per foot");
        LineWords lw;
        RunReads  rd;
        RunSplits sp;
        lw.lines.resize(feet.size());
        const str_er_line_foot *fp = feet.empty() ? nullptr : feet.data();
        const uint32_t         *bp = bits.empty() ? nullptr : bits.data();
        const double           *dp = slopes.empty() ? nullptr : slopes.data();
        str_er_line_words      *lp = lw.lines.empty() ? nullptr : lw.lines.data();
        int32_t nr = 0, nw = 0, np = 0;
        check(str_er_feet_read(ctx_.get(), width, height, fp, bp, dp, (int32_t)feet.size(), lp, nullptr, 0, &nr, nullptr, 0, &nw, nullptr, nullptr));      // (counts)
        const size_t cap = 9 * (size_t)nr + 1;                            // (a run has at most 9 pieces)
        if (cap > 0x7FFFFFFFull) throw std::invalid_argument("feet_split: too many runs");
        lw.runs.resize((size_t)nr + 1);
        lw.words.resize((size_t)nw + 1);
        rd.reads.resize(want_reads ? (size_t)nr + 1 : 0);
        rd.features.resize(1800 * ((size_t)nr + 1));
        sp.splits.resize((size_t)nr + 1);
        sp.pieces.resize(cap);
        sp.piece_reads.resize(want_reads ? cap : 0);
        sp.piece_features.resize(1800 * cap);
        check(str_er_feet_split(ctx_.get(), width, height, fp, bp, dp, (int32_t)feet.size(), lp, lw.runs.data(), nr + 1, &nr, lw.words.data(), nw + 1, &nw,
                                want_reads ? rd.reads.data() : nullptr, rd.features.data(), sp.splits.data(), sp.pieces.data(), (int32_t)cap, &np,
                                want_reads ? sp.piece_reads.data() : nullptr, sp.piece_features.data()));
        lw.runs.resize((size_t)nr);
        lw.words.resize((size_t)nw);
        if (want_reads) rd.reads.resize((size_t)nr);
        rd.features.resize(1800 * (size_t)nr);
        sp.splits.resize((size_t)nr);
        sp.pieces.resize((size_t)np);
        if (want_reads) sp.piece_reads.resize((size_t)np);
        sp.piece_features.resize(1800 * (size_t)np);
        return {std::move(lw), std::move(rd), std::move(sp)};
    }
    // the segmentation of the runs of the words [first_run[w], first_run[w] + n_runs[w]) on the caller's cost rows (str_er_split_words):
    // splits one record per run, run_costs and piece_costs 65 bytes a row.  Returns word_splits, parts and part_costs (the parts' rows,
    // which match_words / decode_words take with first_part and n_parts as the words' spans)
    RunSplits split_words(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                          const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs)
    {
        if (first_run.size() != n_runs.size() || run_costs.size() != 65 * splits.size() || piece_costs.size() % 65)
            throw std::invalid_argument("split_words: 65 bytes a run and a piece, one record a run, one span a word");
        size_t cap = 1;
        for (const int32_t k : n_runs) cap += 4 * (size_t)(k > 0 ? k : 0);          // (a run has at most 4 parts)
        if (cap > 0x7FFFFFFFull) throw std::invalid_argument("split_words: too many runs");
        RunSplits out;
        out.word_splits.resize(first_run.size());
        out.parts.resize(cap);
        out.part_costs.resize(65 * cap);
        int32_t n = 0;
        check(str_er_split_words(ctx_.get(), splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                 piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65), first_run.empty() ? nullptr : first_run.data(),
                                 n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(), out.word_splits.empty() ? nullptr : out.word_splits.data(),
                                 out.parts.data(), (int32_t)cap, &n, out.part_costs.data()));
        out.parts.resize((size_t)n);
        out.part_costs.resize(65 * (size_t)n);
        return out;
    }
    // the string of the split sequence of word w: per part the character of the first minimum of its cost row
    static std::string word_split_text(const RunSplits &sp, size_t w)
    {
        std::string s;
        const str_er_word_split &W = sp.word_splits.at(w);
        for (int32_t k = W.first_part; k < W.first_part + W.n_parts; ++k) {
            const str_er_split_part &P = sp.parts.at((size_t)k);
            const uint8_t *row = P.piece < 0 ? &sp.run_costs.at(65 * (size_t)P.run) : &sp.piece_costs.at(65 * (size_t)P.piece);
            int best = 0;
            for (int a = 1; a < 65; ++a) best = row[a] < row[best] ? a : best;
            s += (char)str_er_ocr_char(best);
        }
        return s;
    }
    // the split text of line t: its words' split strings joined by one blank
    static std::string line_split_text(const LineWords &lw, const RunSplits &sp, size_t t)
    {
        std::string s;
        const str_er_line_words &L = lw.lines.at(t);
        for (int32_t k = L.first_word; k < L.first_word + L.n_words; ++k) s += (k > L.first_word ? " " : "") + word_split_text(sp, (size_t)k);
        return s;
    }

    // Every word decoded jointly over the lattice of the pieces of its runs and the bigram table (STR_ER_WANT_LATTICE_DECODE; the contract
    // is at str_er_lattice_decode in include/str_er.h): one record per word of LineWords::words, 64 label bytes and 64 source bytes per
    // word (0xFF past n_chars; a source indexes the word's lattice parts), and the lattice parts of the words back to back in word order
    // (piece -1: the whole run; the indices are those of RunSplits::parts).  Needs STR_ER_WANT_RUN_SPLIT and a table in the context.
    struct LatticeDecodes {
        std::vector<str_er_lattice_decode> decodes;
        std::vector<uint8_t>               chars, src;
        std::vector<str_er_split_part>     parts;
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static LatticeDecodes lattice_decodes(const str_er_result *r)
    {
        LatticeDecodes out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_lattice_decode *p = str_er_result_lattice_decodes(r, &n)) out.decodes.assign(p, p + n);
        if (const uint8_t *p = str_er_result_lattice_decode_chars(r, &nb)) out.chars.assign(p, p + nb);
        if (const uint8_t *p = str_er_result_lattice_decode_src(r, &nb)) out.src.assign(p, p + nb);
        if (const str_er_split_part *p = str_er_result_lattice_parts(r, &n)) out.parts.assign(p, p + n);
        return out;
    }
    // the joint decode of the words [first_run[w], first_run[w] + n_runs[w]) on the caller's unfolded cost rows (str_er_lattice_decode_words):
    // splits one record per run, run_costs and piece_costs 65 bytes a row; the context's table, INS / DEL and SPLIT
    LatticeDecodes lattice_decode_words(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                                        const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs)
    {
        LatticeDecodes out = lattice_out(splits, run_costs, piece_costs, first_run, n_runs);
        int32_t n = 0;
        check(str_er_lattice_decode_words(ctx_.get(), splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                          piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65),
                                          first_run.empty() ? nullptr : first_run.data(), n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(),
                                          out.decodes.empty() ? nullptr : out.decodes.data(), out.chars.empty() ? nullptr : out.chars.data(),
                                          out.src.empty() ? nullptr : out.src.data(), out.parts.data(), (int32_t)out.parts.size(), &n));
        out.parts.resize((size_t)n);
        return out;
    }
    // the same rules on one host thread, with the table (66 x 66 bytes), INS / DEL and SPLIT as arguments (str_er_lattice_decode_words_host)
    static LatticeDecodes lattice_decode_words_host(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs,
                                                    const std::vector<uint8_t> &piece_costs, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs,
                                                    const std::vector<uint8_t> &table, int32_t ins = 0, int32_t del = 0, int32_t split_cost = 8)
    {
        if (table.size() != 66 * 66) throw std::invalid_argument("lattice_decode_words_host: 66 x 66 bytes");
        LatticeDecodes out = lattice_out(splits, run_costs, piece_costs, first_run, n_runs);
        int32_t n = 0;
        if (str_er_lattice_decode_words_host(splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                             piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65),
                                             first_run.empty() ? nullptr : first_run.data(), n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(),
                                             split_cost, table.data(), ins, del, out.decodes.empty() ? nullptr : out.decodes.data(),
                                             out.chars.empty() ? nullptr : out.chars.data(), out.src.empty() ? nullptr : out.src.data(), out.parts.data(),
                                             (int32_t)out.parts.size(), &n) != STR_ER_OK)
            throw std::invalid_argument("lattice_decode_words_host");
        out.parts.resize((size_t)n);
        return out;
    }
    // The joint decode of lines over the piece lattices of their runs (str_er_lattice_decode_lines; the contract is at
    // str_er_line_lattice_decode in include/str_er.h): one record per line; labels (65: a blank) and sources in slices of 3 entries per
    // node at the line's node slot (the atoms of all runs before its first run), 0xFF / 0xFFFF where nothing is written; the parts of the
    // lines back to back and, per part, the number of breaks before it (-1: dropped)
    struct LineLatticeDecodes {
        std::vector<str_er_line_lattice_decode> decodes;
        std::vector<uint8_t>                    chars;
        std::vector<uint16_t>                   src;
        std::vector<str_er_split_part>          parts;
        std::vector<int32_t>                    word_of_part;
    };
    // whether a detect call with STR_ER_WANT_LATTICE_DECODE also decodes its lines so, and the weight (0 .. 127) of the gap costs
    // (str_er_set_line_lattice_decode; off by default)
    void set_line_lattice_decode(bool on, int32_t weight = 16) { check(str_er_set_line_lattice_decode(ctx_.get(), on ? 1 : 0, weight)); }
    // the tables of such a call, the gap costs used (2 bytes a run) and the lines' windows (first run, run count) with them (all empty
    // when it made none)
    struct LineLatticeResult {
        LineLatticeDecodes   tables;
        std::vector<uint8_t> gap_costs;
        std::vector<int32_t> windows;
    };
    static LineLatticeResult line_lattice_decodes(const str_er_result *r)
    {
        LineLatticeResult out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_line_lattice_decode *p = str_er_result_line_lattice_decodes(r, &n)) out.tables.decodes.assign(p, p + n);
        if (const uint8_t *p = str_er_result_line_lattice_chars(r, &nb)) out.tables.chars.assign(p, p + nb);
        if (const uint16_t *p = str_er_result_line_lattice_src(r, &nb)) out.tables.src.assign(p, p + nb);
        if (const str_er_split_part *p = str_er_result_line_lattice_parts(r, &n)) out.tables.parts.assign(p, p + n);
        if (const int32_t *p = str_er_result_line_lattice_word_of_part(r, &nb)) out.tables.word_of_part.assign(p, p + nb);
        if (const uint8_t *p = str_er_result_line_lattice_gap_costs(r, &nb)) out.gap_costs.assign(p, p + nb);
        if (const int32_t *p = str_er_result_line_lattice_windows(r, &nb)) out.windows.assign(p, p + nb);
        return out;
    }
    // the lines [first_run[t], first_run[t] + n_runs[t]) on the caller's unfolded cost rows: splits one record per run, run_costs and
    // piece_costs 65 bytes a row, gaps 2 bytes a run; the context's table, INS / DEL and SPLIT
    LineLatticeDecodes lattice_decode_lines(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                                            const std::vector<uint8_t> &gaps, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs)
    {
        LineLatticeDecodes out = line_lattice_out(splits, run_costs, piece_costs, gaps, first_run, n_runs);
        int32_t n = 0;
        check(str_er_lattice_decode_lines(ctx_.get(), splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                          piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65), gaps.empty() ? nullptr : gaps.data(),
                                          first_run.empty() ? nullptr : first_run.data(), n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(),
                                          out.decodes.empty() ? nullptr : out.decodes.data(), out.chars.data(), out.src.data(), out.parts.data(),
                                          (int32_t)out.parts.size(), &n, out.word_of_part.data()));
        line_lattice_trim(out, n);
        return out;
    }
    // the same rules on one host thread, with the table (66 x 66 bytes), INS / DEL and SPLIT as arguments (str_er_lattice_decode_lines_host)
    static LineLatticeDecodes lattice_decode_lines_host(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs,
                                                        const std::vector<uint8_t> &piece_costs, const std::vector<uint8_t> &gaps, const std::vector<int32_t> &first_run,
                                                        const std::vector<int32_t> &n_runs, const std::vector<uint8_t> &table, int32_t ins = 0, int32_t del = 0,
                                                        int32_t split_cost = 8)
    {
        if (table.size() != 66 * 66) throw std::invalid_argument("lattice_decode_lines_host: 66 x 66 bytes");
        LineLatticeDecodes out = line_lattice_out(splits, run_costs, piece_costs, gaps, first_run, n_runs);
        int32_t n = 0;
        if (str_er_lattice_decode_lines_host(splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                             piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65), gaps.empty() ? nullptr : gaps.data(),
                                             first_run.empty() ? nullptr : first_run.data(), n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(),
                                             split_cost, table.data(), ins, del, out.decodes.empty() ? nullptr : out.decodes.data(), out.chars.data(), out.src.data(),
                                             out.parts.data(), (int32_t)out.parts.size(), &n, out.word_of_part.data()) != STR_ER_OK)
            throw std::invalid_argument("lattice_decode_lines_host");
        line_lattice_trim(out, n);
        return out;
    }
    // the bytes of the line lattice decoder's back-pointer table on the device (str_er_line_lattice_decode_stats)
    uint64_t line_lattice_decode_table_bytes() const
    {
        uint64_t b = 0;
        check(str_er_line_lattice_decode_stats(ctx_.get(), &b));
        return b;
    }
    // The margins of the jointly decoded words (str_er_set_lattice_margin beside STR_ER_WANT_LATTICE_DECODE; the contract is at
    // str_er_lattice_margin in include/str_er.h): one record per word, and per word 32 reading margins and 32 cut margins (-1 past its
    // parts), 32 readings, 32 alternatives and 32 cut alternatives (0xFF past its parts; 65: the part dropped; a cut alternative is
    // i | j << 4); the edge minima (32 x 4 per word) and the marginals (32 x 4 x 66 per word) only from lattice_margins on the caller's rows
    struct LatticeMargins {
        std::vector<str_er_lattice_margin> margins;
        std::vector<int32_t>               read_margins, cut_margins, edge_min, marginals;
        std::vector<uint8_t>               reads, alts, cut_alts;
    };
    // whether a call with STR_ER_WANT_LATTICE_DECODE also makes the margins (str_er_set_lattice_margin; off by default)
    void set_lattice_margin(bool on) { check(str_er_set_lattice_margin(ctx_.get(), on ? 1 : 0)); }
    // ... copied out of the result of such a call (all empty when it made none)
    static LatticeMargins lattice_margins(const str_er_result *r)
    {
        LatticeMargins out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_lattice_margin *p = str_er_result_lattice_margins(r, &n)) out.margins.assign(p, p + n);
        if (const int32_t *p = str_er_result_lattice_read_margins(r, &nb)) out.read_margins.assign(p, p + nb / 4);
        if (const int32_t *p = str_er_result_lattice_cut_margins(r, &nb)) out.cut_margins.assign(p, p + nb / 4);
        if (const uint8_t *p = str_er_result_lattice_part_reads(r, &nb)) out.reads.assign(p, p + nb);
        if (const uint8_t *p = str_er_result_lattice_part_alts(r, &nb)) out.alts.assign(p, p + nb);
        if (const uint8_t *p = str_er_result_lattice_cut_alts(r, &nb)) out.cut_alts.assign(p, p + nb);
        return out;
    }
    // the margins of the words lattice_decode_words takes, on the caller's unfolded cost rows under the context's table and settings
    // (str_er_lattice_margins)
    LatticeMargins lattice_margins(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                                   const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs, bool edges = false, bool marginals = false)
    {
        if (first_run.size() != n_runs.size() || run_costs.size() != 65 * splits.size() || piece_costs.size() % 65)
            throw std::invalid_argument("lattice_margins: 65 bytes a run and a piece, one record a run, one span a word");
        const size_t   n = first_run.size();
        LatticeMargins out;
        out.margins.resize(n);
        out.read_margins.resize(32 * n);
        out.cut_margins.resize(32 * n);
        out.reads.resize(32 * n);
        out.alts.resize(32 * n);
        out.cut_alts.resize(32 * n);
        if (edges) out.edge_min.resize(32 * 4 * n);
        if (marginals) out.marginals.resize(32 * 4 * 66 * n);
        check(str_er_lattice_margins(ctx_.get(), splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                     piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65), n ? first_run.data() : nullptr,
                                     n ? n_runs.data() : nullptr, (int32_t)n, n ? out.margins.data() : nullptr, n ? out.read_margins.data() : nullptr,
                                     n ? out.cut_margins.data() : nullptr, n ? out.reads.data() : nullptr, n ? out.alts.data() : nullptr,
                                     n ? out.cut_alts.data() : nullptr, edges && n ? out.edge_min.data() : nullptr, marginals && n ? out.marginals.data() : nullptr));
        return out;
    }
    // the jointly decoded string of word w: its own reading where it was not decoded (more than 32 atoms)
    static std::string word_lattice_text(const LineWords &lw, const RunReads &rd, const LatticeDecodes &ld, size_t w)
    {
        const str_er_lattice_decode &d = ld.decodes.at(w);
        if (d.cost < 0) return word_text(lw, rd, w);
        std::string s;
        for (int32_t k = 0; k < d.n_chars; ++k) s += (char)str_er_ocr_char(ld.chars.at(64 * w + (size_t)k));
        return s;
    }
    // the jointly decoded text of line t: its words' strings joined by one blank
    static std::string line_lattice_text(const LineWords &lw, const RunReads &rd, const LatticeDecodes &ld, size_t t)
    {
        std::string s;
        const str_er_line_words &L = lw.lines.at(t);
        for (int32_t k = L.first_word; k < L.first_word + L.n_words; ++k) s += (k > L.first_word ? " " : "") + word_lattice_text(lw, rd, ld, (size_t)k);
        return s;
    }

    // Every word matched against the lexicon over the lattice of the pieces of its runs (STR_ER_WANT_LATTICE_MATCH; the contract is at
    // str_er_lattice_match in include/str_er.h): one record per word of LineWords::words, 32 source bytes per word (0xFF past the winning
    // entry; a source indexes the word's parts) and the parts of the winning entries back to back in word order (piece -1: the whole run;
    // the indices are those of RunSplits::parts).  Needs STR_ER_WANT_RUN_SPLIT, STR_ER_WANT_WORD_MATCH and a lexicon in the context.
    struct LatticeMatches {
        std::vector<str_er_lattice_match> matches;
        std::vector<uint8_t>              src;
        std::vector<str_er_split_part>    parts;
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static LatticeMatches lattice_matches(const str_er_result *r)
    {
        LatticeMatches out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_lattice_match *p = str_er_result_lattice_matches(r, &n)) out.matches.assign(p, p + n);
        if (const uint8_t *p = str_er_result_lattice_match_src(r, &nb)) out.src.assign(p, p + nb);
        if (const str_er_split_part *p = str_er_result_lattice_match_parts(r, &n)) out.parts.assign(p, p + n);
        return out;
    }
    // the lattice match of the words [first_run[w], first_run[w] + n_runs[w]) on the caller's cost rows (str_er_lattice_match_words): splits
    // one record per run, run_costs and piece_costs 65 bytes a row; the context's lexicon, INS / DEL / band and SPLIT
    LatticeMatches lattice_match_words(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                                       const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs)
    {
        LatticeMatches out = lattice_match_out(splits, run_costs, piece_costs, first_run, n_runs);
        int32_t n = 0;
        check(str_er_lattice_match_words(ctx_.get(), splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                         piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65),
                                         first_run.empty() ? nullptr : first_run.data(), n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(),
                                         out.matches.empty() ? nullptr : out.matches.data(), out.src.empty() ? nullptr : out.src.data(), out.parts.data(),
                                         (int32_t)out.parts.size(), &n));
        out.parts.resize((size_t)n);
        return out;
    }
    // the same rules on one host thread, with the lexicon, INS / DEL / band and SPLIT as arguments (str_er_lattice_match_words_host)
    static LatticeMatches lattice_match_words_host(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs,
                                                   const std::vector<uint8_t> &piece_costs, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs,
                                                   const std::vector<std::string> &lexicon, bool fold_case = true, int32_t ins = 64, int32_t del = 64, int32_t band = 2,
                                                   int32_t split_cost = 8)
    {
        std::string          bytes;
        std::vector<int32_t> offsets{0};
        for (const std::string &w : lexicon) {
            bytes += w;
            if (bytes.size() > (size_t)INT32_MAX) throw std::invalid_argument("lattice_match_words_host: too many bytes");
            offsets.push_back((int32_t)bytes.size());
        }
        LatticeMatches out = lattice_match_out(splits, run_costs, piece_costs, first_run, n_runs);
        int32_t n = 0;
        if (str_er_lattice_match_words_host(splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                            piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65),
                                            first_run.empty() ? nullptr : first_run.data(), n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(),
                                            bytes.data(), offsets.data(), (int32_t)lexicon.size(), fold_case ? STR_ER_LEXICON_FOLD_CASE : 0u, ins, del, band, split_cost,
                                            out.matches.empty() ? nullptr : out.matches.data(), out.src.empty() ? nullptr : out.src.data(), out.parts.data(),
                                            (int32_t)out.parts.size(), &n) != STR_ER_OK)
            throw std::invalid_argument("lattice_match_words_host");
        out.parts.resize((size_t)n);
        return out;
    }
    // the string of word w matched over its piece lattice: the lexicon entry (as given in `lexicon`) that matches it best, its own reading
    // where none does
    static std::string word_lattice_match_text(const LineWords &lw, const RunReads &rd, const LatticeMatches &lm, const std::vector<std::string> &lexicon, size_t w)
    {
        const int32_t e = lm.matches.at(w).entry;
        return e >= 0 && (size_t)e < lexicon.size() ? lexicon[(size_t)e] : word_text(lw, rd, w);
    }
    // the text of line t matched over the piece lattices: its words' strings joined by one blank
    static std::string line_lattice_match_text(const LineWords &lw, const RunReads &rd, const LatticeMatches &lm, const std::vector<std::string> &lexicon, size_t t)
    {
        std::string s;
        const str_er_line_words &L = lw.lines.at(t);
        for (int32_t k = L.first_word; k < L.first_word + L.n_words; ++k)
            s += (k > L.first_word ? " " : "") + word_lattice_match_text(lw, rd, lm, lexicon, (size_t)k);
        return s;
    }

    // The track match over the members' piece lattices of a detect call made with STR_ER_WANT_LATTICE_TRACK (needs STR_ER_WANT_TRACK_READ and
    // STR_ER_WANT_LATTICE_MATCH; the contract is at str_er_lattice_track_member in include/str_er.h): one record per word track, one member
    // record and 32 source bytes per slot of the word tracks' member array, and the members' parts back to back in slot order
    struct LatticeTrackMatches {
        std::vector<str_er_track_match>          matches;
        std::vector<str_er_lattice_track_member> members;
        std::vector<uint8_t>                     src;
        std::vector<str_er_split_part>           parts;
    };
    static LatticeTrackMatches lattice_track_matches(const str_er_result *r)
    {
        LatticeTrackMatches out;
        int32_t  n = 0;
        uint64_t nb = 0;
        if (const str_er_track_match *p = str_er_result_lattice_track_matches(r, &n)) out.matches.assign(p, p + n);
        if (const str_er_lattice_track_member *p = str_er_result_lattice_track_members(r, &n)) out.members.assign(p, p + n);
        if (const uint8_t *p = str_er_result_lattice_track_src(r, &nb)) out.src.assign(p, p + nb);
        if (const str_er_split_part *p = str_er_result_lattice_track_parts(r, &n)) out.parts.assign(p, p + n);
        return out;
    }
    // the same match of the tracks members[track_first[g] .. track_first[g] + track_count[g]) of the words [first_run[w], first_run[w] +
    // n_runs[w]) on the caller's rows (str_er_lattice_match_tracks): the context's lexicon, INS / DEL / band and SPLIT
    LatticeTrackMatches lattice_match_tracks(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                                             const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs, const std::vector<int32_t> &track_first,
                                             const std::vector<int32_t> &track_count, const std::vector<int32_t> &members)
    {
        LatticeTrackMatches out = lattice_track_out(splits, run_costs, piece_costs, first_run, n_runs, track_first, track_count, members);
        int32_t n = 0;
        check(str_er_lattice_match_tracks(ctx_.get(), splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                          piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65),
                                          first_run.empty() ? nullptr : first_run.data(), n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(),
                                          track_first.empty() ? nullptr : track_first.data(), track_count.empty() ? nullptr : track_count.data(),
                                          members.empty() ? nullptr : members.data(), (int32_t)members.size(), (int32_t)track_first.size(),
                                          out.matches.empty() ? nullptr : out.matches.data(), out.members.empty() ? nullptr : out.members.data(),
                                          out.src.empty() ? nullptr : out.src.data(), out.parts.data(), (int32_t)out.parts.size(), &n));
        out.parts.resize((size_t)n);
        return out;
    }
    // the same rules on one host thread, with the lexicon, INS / DEL / band and SPLIT as arguments (str_er_lattice_match_tracks_host)
    static LatticeTrackMatches lattice_match_tracks_host(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs,
                                                         const std::vector<uint8_t> &piece_costs, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs,
                                                         const std::vector<int32_t> &track_first, const std::vector<int32_t> &track_count,
                                                         const std::vector<int32_t> &members, const std::vector<std::string> &lexicon, bool fold_case = true,
                                                         int32_t ins = 64, int32_t del = 64, int32_t band = 2, int32_t split_cost = 8)
    {
        std::string          bytes;
        std::vector<int32_t> offsets{0};
        for (const std::string &w : lexicon) {
            bytes += w;
            if (bytes.size() > (size_t)INT32_MAX) throw std::invalid_argument("lattice_match_tracks_host: too many bytes");
            offsets.push_back((int32_t)bytes.size());
        }
        LatticeTrackMatches out = lattice_track_out(splits, run_costs, piece_costs, first_run, n_runs, track_first, track_count, members);
        int32_t n = 0;
        if (str_er_lattice_match_tracks_host(splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                             piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65),
                                             first_run.empty() ? nullptr : first_run.data(), n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(),
                                             track_first.empty() ? nullptr : track_first.data(), track_count.empty() ? nullptr : track_count.data(),
                                             members.empty() ? nullptr : members.data(), (int32_t)members.size(), (int32_t)track_first.size(), bytes.data(),
                                             offsets.data(), (int32_t)lexicon.size(), fold_case ? STR_ER_LEXICON_FOLD_CASE : 0u, ins, del, band, split_cost,
                                             out.matches.empty() ? nullptr : out.matches.data(), out.members.empty() ? nullptr : out.members.data(),
                                             out.src.empty() ? nullptr : out.src.data(), out.parts.data(), (int32_t)out.parts.size(), &n) != STR_ER_OK)
            throw std::invalid_argument("lattice_match_tracks_host");
        out.parts.resize((size_t)n);
        return out;
    }
    // The decode of the same tracks over their members' piece lattices, without a lexicon (str_er_lattice_decode_tracks; the contract is
    // at str_er_lattice_track_decode in include/str_er.h): the context's table, str_er_set_word_decode INS / DEL for the seeds,
    // str_er_set_track_decode parameters and SPLIT.  Per track a record and 32 labels, per slot of the member array a record and 32
    // source bytes, and the members' parts back to back.
    struct LatticeTrackDecodes {
        std::vector<str_er_track_decode>         decodes;
        std::vector<uint8_t>                     chars;
        std::vector<str_er_lattice_track_member> members;
        std::vector<uint8_t>                     src;
        std::vector<str_er_split_part>           parts;
    };
    LatticeTrackDecodes lattice_decode_tracks(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                                              const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs, const std::vector<int32_t> &track_first,
                                              const std::vector<int32_t> &track_count, const std::vector<int32_t> &members)
    {
        LatticeTrackMatches sized = lattice_track_out(splits, run_costs, piece_costs, first_run, n_runs, track_first, track_count, members);
        LatticeTrackDecodes out;
        out.decodes.resize(track_first.size()); out.chars.assign(32 * track_first.size(), 0xFF);
        out.members.swap(sized.members); out.src.swap(sized.src); out.parts.swap(sized.parts);
        int32_t n = 0;
        check(str_er_lattice_decode_tracks(ctx_.get(), splits.empty() ? nullptr : splits.data(), (int32_t)splits.size(), run_costs.empty() ? nullptr : run_costs.data(),
                                           piece_costs.empty() ? nullptr : piece_costs.data(), (int32_t)(piece_costs.size() / 65),
                                           first_run.empty() ? nullptr : first_run.data(), n_runs.empty() ? nullptr : n_runs.data(), (int32_t)first_run.size(),
                                           track_first.empty() ? nullptr : track_first.data(), track_count.empty() ? nullptr : track_count.data(),
                                           members.empty() ? nullptr : members.data(), (int32_t)members.size(), (int32_t)track_first.size(),
                                           out.decodes.empty() ? nullptr : out.decodes.data(), out.chars.empty() ? nullptr : out.chars.data(),
                                           out.members.empty() ? nullptr : out.members.data(), out.src.empty() ? nullptr : out.src.data(), out.parts.data(),
                                           (int32_t)out.parts.size(), &n));
        out.parts.resize((size_t)n);
        return out;
    }
    // the string word track g takes over its members' piece lattices: the lexicon entry (as given in `lexicon`), "" where it has none
    static std::string word_track_lattice_text(const LatticeTrackMatches &lt, const std::vector<std::string> &lexicon, size_t g)
    {
        const int32_t e = lt.matches.at(g).entry;
        return e >= 0 && (size_t)e < lexicon.size() ? lexicon[(size_t)e] : std::string();
    }

    // The text lines of consecutive frames linked into text tracks (STR_ER_WANT_LINE_LINKS; the contract is at str_er_line_link in
    // include/str_er.h): the overlaps across adjacent frames, the track of every line of str_er_result_texts(), the tracks, the line
    // indices their first / count index, and the footprints of the lines of the first ([0]) and of the last frame ([1]).
    struct EdgeFeet {
        int32_t width = 0, height = 0;               // the frame's size
        std::vector<int32_t>          lines;         // indices into str_er_result_texts()
        std::vector<str_er_line_foot> feet;
        std::vector<uint32_t>         bits;          // rows of (w + 31) / 32 words over every foot box, back to back
    };
    struct LineLinks {
        std::vector<str_er_line_link>  links;
        std::vector<int32_t>           line_tracks;
        std::vector<str_er_text_track> tracks;
        std::vector<int32_t>           members;
        EdgeFeet                       edge[2];
    };
    // ... copied out of the result of a call with the flag (all empty without it)
    static LineLinks line_links(const str_er_result *r)
    {
        LineLinks out;
        int32_t n = 0;
        if (const str_er_line_link *p = str_er_result_line_links(r, &n)) out.links.assign(p, p + n);
        if (const int32_t *p = str_er_result_line_tracks(r, &n)) out.line_tracks.assign(p, p + n);
        if (const str_er_text_track *p = str_er_result_text_tracks(r, &n)) out.tracks.assign(p, p + n);
        if (const int32_t *p = str_er_result_text_track_members(r, &n)) out.members.assign(p, p + n);
        for (int which = 0; which < 2; ++which) {
            const str_er_line_foot *feet = nullptr;
            const int32_t  *lines = nullptr;
            const uint32_t *bits = nullptr;
            uint64_t n_words = 0;
            EdgeFeet &e = out.edge[which];
            if (str_er_result_edge_feet(r, which, &e.width, &e.height, &feet, &lines, &n, &bits, &n_words) != STR_ER_OK) continue;
            e.lines.assign(lines, lines + n); e.feet.assign(feet, feet + n); e.bits.assign(bits, bits + n_words);
        }
        return out;
    }
    // two lines of adjacent frames are linked from a Jaccard index of num / den of their footprints on (str_er_set_line_link)
    void set_line_link(int num, int den) { check(str_er_set_line_link(ctx_.get(), num, den)); }
    // the overlaps of every line of a with every line of b, two sets of footprints of one frame size (str_er_link_feet): a / b of a
    // record index the two sets, link is set at the context's threshold
    std::vector<str_er_line_link> link_feet(const EdgeFeet &a, const EdgeFeet &b) { return link_feet(ctx_.get(), a, b); }
    static std::vector<str_er_line_link> link_feet(str_er_ctx *ctx, const EdgeFeet &a, const EdgeFeet &b)
    {
        if (a.width != b.width || a.height != b.height || a.feet.empty() || b.feet.empty()) return {};      // (another frame size: not adjacent)
        int32_t n = 0;
        const uint32_t *ba = a.bits.empty() ? nullptr : a.bits.data(), *bb = b.bits.empty() ? nullptr : b.bits.data();
        const auto run = [&](str_er_line_link *out, int32_t cap) {
            return str_er_link_feet(ctx, a.width, a.height, a.feet.data(), ba, (int32_t)a.feet.size(), b.feet.data(), bb, (int32_t)b.feet.size(), out, cap, &n);
        };
        if (run(nullptr, 0) != STR_ER_OK) throw std::runtime_error(std::string("str_er_link_feet: ") + str_er_last_error(ctx));
        std::vector<str_er_line_link> out((size_t)n);
        if (n && run(out.data(), n) != STR_ER_OK) throw std::runtime_error(std::string("str_er_link_feet: ") + str_er_last_error(ctx));
        return out;
    }
    // Persistent track ids over the results of consecutive calls or stream submissions, fed in time order: update() links the last
    // frame of the previous result with the first frame of this one and returns an id per line.  A track that continues keeps its
    // id; two tracks a later result joins keep the smaller one (resolve() maps an id handed out earlier to its current one).
    class TextTracker {
    public:
        // linker: the context whose str_er_link_feet (and threshold) links the two results
        std::vector<int64_t> update(str_er_ctx *linker, const LineLinks &res)
        {
            const int64_t base = (int64_t)parent_.size();
            for (size_t i = 0; i < res.tracks.size(); ++i) parent_.push_back(base + (int64_t)i);
            if (have_prev_)
                for (const str_er_line_link &k : link_feet(linker, prev_, res.edge[0]))
                    if (k.link) join(prev_ids_[(size_t)k.a], base + res.line_tracks[(size_t)res.edge[0].lines[(size_t)k.b]]);
            std::vector<int64_t> ids(res.line_tracks.size());
            for (size_t t = 0; t < ids.size(); ++t) ids[t] = resolve(base + res.line_tracks[t]);
            prev_ = res.edge[1];
            prev_ids_.clear();
            for (const int32_t t : prev_.lines) prev_ids_.push_back(ids[(size_t)t]);
            have_prev_ = true;
            return ids;
        }
        int64_t resolve(int64_t id)
        {
            while (parent_[(size_t)id] != id) { parent_[(size_t)id] = parent_[(size_t)parent_[(size_t)id]]; id = parent_[(size_t)id]; }
            return id;
        }
        void reset() { have_prev_ = false; }
    private:
        void join(int64_t a, int64_t b)
        {
            a = resolve(a); b = resolve(b);
            if (a != b) parent_[(size_t)std::max(a, b)] = std::min(a, b);
        }
        std::vector<int64_t> parent_, prev_ids_;
        EdgeFeet prev_;
        bool     have_prev_ = false;
    };

    // The track pool (str_er_track_pool_*; the contract is at str_er_pool_match in include/str_er.h): cap_tracks pooled word tracks
    // on the device, per slot the summed costs of everything added to it against every entry of the filter's lexicon, kept from call
    // to call.  Bound to the lexicon, INS / DEL / band and (lattice) SPLIT of the filter as they are at creation: after one of their
    // setters every call throws (STR_ER_ESTATE) until reset().  The pool keeps its context alive.
    class TrackPool {
    public:
        TrackPool(const ERFilter &f, int32_t cap_tracks, bool lattice = false) : ctx_(f.ctx_)
        {
            str_er_track_pool *p = nullptr;
            check(str_er_track_pool_create(ctx_.get(), cap_tracks, lattice ? STR_ER_POOL_LATTICE : 0u, &p));
            pool_.reset(p, str_er_track_pool_destroy);
        }
        // the tracks, given as for match_tracks, are added to the slots slots[g] (distinct)
        void add(const std::vector<uint8_t> &costs, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs, const std::vector<int32_t> &track_first,
                 const std::vector<int32_t> &track_count, const std::vector<int32_t> &members, const std::vector<int32_t> &slots)
        {
            if (costs.size() % 65 || first_run.size() != n_runs.size() || track_first.size() != track_count.size() || slots.size() != track_first.size())
                throw std::invalid_argument("TrackPool::add: 65 bytes a run, one span a word, one span and one slot a track");
            check(str_er_track_pool_add(pool_.get(), ptr(costs), (int32_t)(costs.size() / 65), ptr(first_run), ptr(n_runs), (int32_t)first_run.size(), ptr(track_first),
                                        ptr(track_count), ptr(members), (int32_t)members.size(), (int32_t)track_first.size(), ptr(slots)));
        }
        // ... for a lattice pool, the tracks given as for lattice_match_tracks
        void add_lattice(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                         const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs, const std::vector<int32_t> &track_first,
                         const std::vector<int32_t> &track_count, const std::vector<int32_t> &members, const std::vector<int32_t> &slots)
        {
            if (run_costs.size() != 65 * splits.size() || piece_costs.size() % 65 || first_run.size() != n_runs.size() || track_first.size() != track_count.size() ||
                slots.size() != track_first.size())
                throw std::invalid_argument("TrackPool::add_lattice: 65 bytes a run and a piece, one record a run, one span a word, one span and one slot a track");
            check(str_er_track_pool_add_lattice(pool_.get(), ptr(splits), (int32_t)splits.size(), ptr(run_costs), ptr(piece_costs), (int32_t)(piece_costs.size() / 65),
                                                ptr(first_run), ptr(n_runs), (int32_t)first_run.size(), ptr(track_first), ptr(track_count), ptr(members),
                                                (int32_t)members.size(), (int32_t)track_first.size(), ptr(slots)));
        }
        // slot dst takes the members of the slots srcs, which become empty
        void join(int32_t dst, const std::vector<int32_t> &srcs) { check(str_er_track_pool_join(pool_.get(), dst, ptr(srcs), (int32_t)srcs.size())); }
        void clear(const std::vector<int32_t> &slots) { check(str_er_track_pool_clear(pool_.get(), ptr(slots), (int32_t)slots.size())); }
        // one record per slot named (a slot may be named more than once)
        std::vector<str_er_pool_match> read(const std::vector<int32_t> &slots)
        {
            std::vector<str_er_pool_match> out(slots.size());
            check(str_er_track_pool_read(pool_.get(), ptr(slots), (int32_t)slots.size(), out.empty() ? nullptr : out.data()));
            return out;
        }
        // every slot empty, the pool bound to the filter's lexicon and parameters as they are now
        void reset() { check(str_er_track_pool_reset(pool_.get())); }
        struct Info {
            int32_t  cap_tracks = 0;
            uint32_t flags = 0;
            int32_t  n_entries = 0;
            uint64_t device_bytes = 0;
            int32_t  in_use = 0, stale = 0;
        };
        Info info() const
        {
            Info i;
            check(str_er_track_pool_info(pool_.get(), &i.cap_tracks, &i.flags, &i.n_entries, &i.device_bytes, &i.in_use, &i.stale));
            return i;
        }
    private:
        template <typename T> static const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
        void check(int rc) const
        {
            if (rc != STR_ER_OK) throw std::runtime_error(std::string(str_er_strerror(rc)) + ": " + str_er_last_error(ctx_.get()));
        }
        std::shared_ptr<str_er_ctx>        ctx_;      // (declared first: the pool is destroyed before its context)
        std::shared_ptr<str_er_track_pool> pool_;
    };

    // The decode pool (str_er_track_pool_create_decode; the contract is at str_er_pool_decode in include/str_er.h): cap_tracks pooled
    // word tracks on the device without a lexicon, per slot the newest `keep` usable members added to it -- their cost rows and decoder
    // strings -- kept from call to call; read() decodes a slot as decode_tracks decodes the track of its kept members in age order.
    // Bound to the bigram table, set_word_decode and set_track_decode of the filter as they are at creation: after one of their
    // setters every call throws (STR_ER_ESTATE) until reset().  The pool keeps its context alive.
    class DecodePool {
    public:
        DecodePool(const ERFilter &f, int32_t cap_tracks, int32_t keep = 32) : ctx_(f.ctx_), keep_(keep)
        {
            str_er_track_pool *p = nullptr;
            check(str_er_track_pool_create_decode(ctx_.get(), cap_tracks, keep, &p));
            pool_.reset(p, str_er_track_pool_destroy);
        }
        int32_t keep() const { return keep_; }
        // the tracks, given as for decode_tracks (unfolded rows), are added to the slots slots[g] (distinct)
        void add(const std::vector<uint8_t> &costs, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs, const std::vector<int32_t> &track_first,
                 const std::vector<int32_t> &track_count, const std::vector<int32_t> &members, const std::vector<int32_t> &slots)
        {
            if (costs.size() % 65 || first_run.size() != n_runs.size() || track_first.size() != track_count.size() || slots.size() != track_first.size())
                throw std::invalid_argument("DecodePool::add: 65 bytes a run, one span a word, one span and one slot a track");
            check(str_er_track_pool_add(pool_.get(), ptr(costs), (int32_t)(costs.size() / 65), ptr(first_run), ptr(n_runs), (int32_t)first_run.size(), ptr(track_first),
                                        ptr(track_count), ptr(members), (int32_t)members.size(), (int32_t)track_first.size(), ptr(slots)));
        }
        // slot dst keeps the newest of its own and the srcs' kept members; the srcs become empty
        void join(int32_t dst, const std::vector<int32_t> &srcs) { check(str_er_track_pool_join(pool_.get(), dst, ptr(srcs), (int32_t)srcs.size())); }
        void clear(const std::vector<int32_t> &slots) { check(str_er_track_pool_clear(pool_.get(), ptr(slots), (int32_t)slots.size())); }
        // per slot named (a slot may be named more than once) a record, 32 labels and keep member costs in age order, -1 past n_kept
        struct Reads {
            std::vector<str_er_pool_decode> records;
            std::vector<uint8_t>            chars;
            std::vector<int32_t>            member_costs;
        };
        Reads read(const std::vector<int32_t> &slots)
        {
            Reads r;
            r.records.resize(slots.size()); r.chars.assign(32 * slots.size(), 0xFF); r.member_costs.assign((size_t)keep_ * slots.size(), -1);
            check(str_er_track_pool_read_decode(pool_.get(), ptr(slots), (int32_t)slots.size(), r.records.empty() ? nullptr : r.records.data(),
                                                r.chars.empty() ? nullptr : r.chars.data(), r.member_costs.empty() ? nullptr : r.member_costs.data()));
            return r;
        }
        // the kept list of a slot in age order: keys, run counts and 32 rows of 65 bytes a member
        struct Members {
            std::vector<uint64_t> keys;
            std::vector<int32_t>  n_runs;
            std::vector<uint8_t>  rows;
        };
        Members members(int32_t slot)
        {
            Members m;
            m.keys.resize((size_t)keep_); m.n_runs.resize((size_t)keep_); m.rows.resize((size_t)keep_ * 32 * 65);
            int32_t n = 0;
            check(str_er_track_pool_members(pool_.get(), slot, m.keys.data(), m.n_runs.data(), m.rows.data(), &n));
            m.keys.resize((size_t)n); m.n_runs.resize((size_t)n); m.rows.resize((size_t)n * 32 * 65);
            return m;
        }
        // every slot empty, the pool bound to the filter's table and parameters as they are now
        void reset() { check(str_er_track_pool_reset(pool_.get())); }
    private:
        template <typename T> static const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
        void check(int rc) const
        {
            if (rc != STR_ER_OK) throw std::runtime_error(std::string(str_er_strerror(rc)) + ": " + str_er_last_error(ctx_.get()));
        }
        std::shared_ptr<str_er_ctx>        ctx_;      // (declared first: the pool is destroyed before its context)
        std::shared_ptr<str_er_track_pool> pool_;
        int32_t                            keep_;
    };

    // The lattice decode pool (str_er_track_pool_create_lattice_decode; the contract is at "The lattice decode pool" in
    // include/str_er.h): a decode pool over the members' piece lattices -- per slot the newest `keep` usable members (N <= 32 nodes),
    // their split records, run rows, piece rows and lattice decoder strings, kept from call to call; a read decodes a slot as
    // lattice_decode_tracks decodes the track of its kept members in age order.  Bound to what a DecodePool is bound to and to SPLIT:
    // after one of their setters (set_run_split with another SPLIT) every call throws (STR_ER_ESTATE) until reset().
    class LatticeDecodePool {
    public:
        LatticeDecodePool(const ERFilter &f, int32_t cap_tracks, int32_t keep = 32) : ctx_(f.ctx_), keep_(keep)
        {
            str_er_track_pool *p = nullptr;
            check(str_er_track_pool_create_lattice_decode(ctx_.get(), cap_tracks, keep, &p));
            pool_.reset(p, str_er_track_pool_destroy);
        }
        int32_t keep() const { return keep_; }
        // the tracks, given as for lattice_decode_tracks (unfolded rows), are added to the slots slots[g] (distinct)
        void add_lattice(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                         const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs, const std::vector<int32_t> &track_first,
                         const std::vector<int32_t> &track_count, const std::vector<int32_t> &members, const std::vector<int32_t> &slots)
        {
            if (run_costs.size() != 65 * splits.size() || piece_costs.size() % 65 || first_run.size() != n_runs.size() || track_first.size() != track_count.size() ||
                slots.size() != track_first.size())
                throw std::invalid_argument("LatticeDecodePool::add_lattice: 65 bytes a run and a piece, one record a run, one span a word, one span and one slot a track");
            check(str_er_track_pool_add_lattice(pool_.get(), ptr(splits), (int32_t)splits.size(), ptr(run_costs), ptr(piece_costs), (int32_t)(piece_costs.size() / 65),
                                                ptr(first_run), ptr(n_runs), (int32_t)first_run.size(), ptr(track_first), ptr(track_count), ptr(members),
                                                (int32_t)members.size(), (int32_t)track_first.size(), ptr(slots)));
        }
        // slot dst keeps the newest of its own and the srcs' kept members; the srcs become empty
        void join(int32_t dst, const std::vector<int32_t> &srcs) { check(str_er_track_pool_join(pool_.get(), dst, ptr(srcs), (int32_t)srcs.size())); }
        void clear(const std::vector<int32_t> &slots) { check(str_er_track_pool_clear(pool_.get(), ptr(slots), (int32_t)slots.size())); }
        // per slot named (a slot may be named more than once) a record, 32 labels and keep member costs in age order (-1 past n_kept);
        // keep member records (word: the age rank; cost = word = -1 past n_kept) and 32 source bytes each; the kept members' parts of
        // all slots back to back (run 32 * rank + the member's run, piece 80 * rank + the member's piece row)
        struct Reads {
            std::vector<str_er_pool_decode>          records;
            std::vector<uint8_t>                     chars;
            std::vector<int32_t>                     member_costs;
            std::vector<str_er_lattice_track_member> members;
            std::vector<uint8_t>                     src;
            std::vector<str_er_split_part>           parts;
        };
        Reads read(const std::vector<int32_t> &slots)
        {
            const size_t nk = (size_t)keep_ * slots.size();
            if (32 * nk + 1 > 0x7FFFFFFFull) throw std::invalid_argument("LatticeDecodePool::read: too many slots");
            Reads r;
            r.records.resize(slots.size()); r.chars.assign(32 * slots.size(), 0xFF); r.member_costs.assign(nk, -1);
            r.members.resize(nk); r.src.assign(32 * nk, 0xFF); r.parts.resize(32 * nk + 1);
            int32_t n = 0;
            check(str_er_track_pool_read_lattice_decode(pool_.get(), ptr(slots), (int32_t)slots.size(), ptr(r.records), r.chars.empty() ? nullptr : r.chars.data(),
                                                        r.member_costs.empty() ? nullptr : r.member_costs.data(), r.members.empty() ? nullptr : r.members.data(),
                                                        r.src.empty() ? nullptr : r.src.data(), r.parts.data(), (int32_t)r.parts.size(), &n));
            r.parts.resize((size_t)n);
            return r;
        }
        // the record, the labels and the member costs alone (str_er_track_pool_read_decode: the same decode, less to copy back)
        Reads read_decode(const std::vector<int32_t> &slots)
        {
            Reads r;
            r.records.resize(slots.size()); r.chars.assign(32 * slots.size(), 0xFF); r.member_costs.assign((size_t)keep_ * slots.size(), -1);
            check(str_er_track_pool_read_decode(pool_.get(), ptr(slots), (int32_t)slots.size(), ptr(r.records), r.chars.empty() ? nullptr : r.chars.data(),
                                                r.member_costs.empty() ? nullptr : r.member_costs.data()));
            return r;
        }
        // the kept list of a slot in age order: keys, run counts, and per member 32 split records (first_piece: into its own piece
        // rows), 32 run rows and 80 piece rows of 65 bytes
        struct Members {
            std::vector<uint64_t>         keys;
            std::vector<int32_t>          n_runs;
            std::vector<str_er_run_split> splits;
            std::vector<uint8_t>          run_rows, piece_rows;
        };
        Members members(int32_t slot)
        {
            Members      m;
            const size_t k = (size_t)keep_;
            m.keys.resize(k); m.n_runs.resize(k); m.splits.resize(k * 32); m.run_rows.resize(k * 32 * 65); m.piece_rows.resize(k * 80 * 65);
            int32_t n = 0;
            check(str_er_track_pool_lattice_members(pool_.get(), slot, m.keys.data(), m.n_runs.data(), m.splits.data(), m.run_rows.data(), m.piece_rows.data(), &n));
            m.keys.resize((size_t)n); m.n_runs.resize((size_t)n); m.splits.resize((size_t)n * 32); m.run_rows.resize((size_t)n * 32 * 65);
            m.piece_rows.resize((size_t)n * 80 * 65);
            return m;
        }
        // every slot empty, the pool bound to the filter's table, parameters and SPLIT as they are now
        void reset() { check(str_er_track_pool_reset(pool_.get())); }
    private:
        template <typename T> static const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
        template <typename T> static T *ptr(std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
        void check(int rc) const
        {
            if (rc != STR_ER_OK) throw std::runtime_error(std::string(str_er_strerror(rc)) + ": " + str_er_last_error(ctx_.get()));
        }
        std::shared_ptr<str_er_ctx>        ctx_;      // (declared first: the pool is destroyed before its context)
        std::shared_ptr<str_er_track_pool> pool_;
        int32_t                            keep_;
    };

    // vector<double> ERFilter::make_LBP_hist(Mat input, N = 2, normalize_size = 24) (src/ER.cpp:789-816)
    std::vector<double> make_LBP_hist(const Image8 &input)
    {
        const int32_t box[4] = {0, 0, input.cols, input.rows};
        std::vector<double> h(1024);
        check(str_er_lbp_hist(ctx_.get(), input.data, input.cols, input.rows, input.step, box, 1, h.data(), nullptr));
        return h;
    }

    // Mat ERFilter::calc_LBP(Mat input, const int size = 24) (inc/ER.h:134, src/ER.cpp:819-845): the 24 x 24 code map, row-major
    std::vector<uint8_t> calc_LBP(const Image8 &input)
    {
        const int32_t box[4] = {0, 0, input.cols, input.rows};
        std::vector<uint8_t> lbp(24 * 24);
        check(str_er_calc_lbp(ctx_.get(), input.data, input.cols, input.rows, input.step, box, 1, lbp.data()));
        return lbp;
    }

    // void ERFilter::er_track(vector<ERs> &strong, vector<ERs> &weak, ERs &all_er, vector<Mat> &channel, Mat Ycrcb)
    // (src/ER.cpp:530-590).  channel[i] is the plane strong[i] / weak[i] came from, Ycrcb the 8UC3 image
    // compute_channels made.  all_er = the strong ERs (channel order), then the tracked weak ones in channel / list
    // order (the reference appends them in the order its nested loops find them; er_grouping sorts all_er anyway).
    void er_track(std::vector<ERs> &strong, std::vector<ERs> &weak, ERs &all_er, const std::vector<Image8> &channel, const Image8 &Ycrcb)
    {
        if (Ycrcb.channels != 3) throw std::runtime_error("er_track: Ycrcb must be 8UC3");
        std::vector<ER *> ers;
        std::vector<str_er_cand> cands;
        std::vector<double> colors;
        for (size_t i = 0; i < strong.size(); ++i)
            for (int pass = 0; pass < 2; ++pass) {
                ERs &list = pass == 0 ? strong[i] : weak[i];
                if (list.empty()) continue;
                std::vector<int32_t> boxes;
                for (ER *e : list) { boxes.push_back(e->bound.x); boxes.push_back(e->bound.y); boxes.push_back(e->bound.width); boxes.push_back(e->bound.height); }
                std::vector<double> col(3 * list.size());
                check(str_er_calc_color(ctx_.get(), channel[i].data, channel[i].cols, channel[i].rows, channel[i].step, Ycrcb.data, Ycrcb.cols,
                                        Ycrcb.rows, Ycrcb.step, boxes.data(), (int32_t)list.size(), col.data()));
                for (size_t k = 0; k < list.size(); ++k) {
                    ER *e = list[k];
                    e->color1 = col[3 * k]; e->color2 = col[3 * k + 1]; e->color3 = col[3 * k + 2];
                    e->center.x = e->bound.x + e->bound.width / 2; e->center.y = e->bound.y + e->bound.height / 2;
                    e->ch = (int)i;
                    str_er_cand c{};
                    c.ch = (uint8_t)i; c.cls = pass == 0 ? STR_ER_CLS_STRONG : STR_ER_CLS_WEAK;
                    c.x = (uint16_t)e->bound.x; c.y = (uint16_t)e->bound.y; c.w = (uint16_t)e->bound.width; c.h = (uint16_t)e->bound.height;
                    c.area = (uint32_t)e->area; c.key = e->key;
                    ers.push_back(e); cands.push_back(c);
                    colors.insert(colors.end(), col.begin() + 3 * k, col.begin() + 3 * k + 3);
                }
            }
        std::vector<uint8_t> tracked(ers.size());
        check(str_er_er_track(ctx_.get(), cands.data(), colors.data(), (int32_t)ers.size(), tracked.data(), nullptr, nullptr));
        for (size_t k = 0; k < ers.size(); ++k) if (cands[k].cls == STR_ER_CLS_STRONG) all_er.push_back(ers[k]);
        for (size_t k = 0; k < ers.size(); ++k) if (cands[k].cls == STR_ER_CLS_WEAK && tracked[k]) all_er.push_back(ers[k]);
    }

    // void ERFilter::er_grouping(ERs &all_er, vector<Text> &text, bool overlap_sup, bool inner_sup) (src/ER.cpp:612-692).
    // all_er comes back sorted by center.x (and inner-suppressed); bound / center of ERs that overlap_suppression merged
    // into are updated in place as in the reference, and the ERs it merged away are erased.
    void er_grouping(ERs &all_er, std::vector<Text> &text, bool overlap_sup = false, bool inner_sup = false)
    {
        // ties in center.x are broken by candidate order = (channel, key), whatever order all_er arrives in
        std::sort(all_er.begin(), all_er.end(), [](const ER *a, const ER *b) { return a->ch != b->ch ? a->ch < b->ch : a->key < b->key; });
        const int32_t n = (int32_t)all_er.size();
        std::vector<str_er_cand> cands((size_t)n);
        std::vector<str_er_track> tr((size_t)n);
        for (int32_t k = 0; k < n; ++k) {
            const ER *e = all_er[(size_t)k];
            str_er_cand c{};
            c.x = (uint16_t)e->bound.x; c.y = (uint16_t)e->bound.y; c.w = (uint16_t)e->bound.width; c.h = (uint16_t)e->bound.height;
            c.area = (uint32_t)e->area; c.ch = (uint8_t)e->ch; c.key = e->key;
            cands[(size_t)k] = c;
            str_er_track t{};
            t.color1 = e->color1; t.color2 = e->color2; t.color3 = e->color3; t.cx = e->center.x; t.cy = e->center.y; t.tracked = 1;
            tr[(size_t)k] = t;
        }
        str_er_result *r = nullptr;
        check(str_er_er_grouping(ctx_.get(), cands.data(), tr.data(), n, overlap_sup ? 1 : 0, inner_sup ? 1 : 0, &r));
        std::unique_ptr<str_er_result, void (*)(str_er_result *)> guard(r, str_er_result_free);
        int32_t nt = 0, ne = 0, nb = 0;
        const str_er_text   *tx = str_er_result_texts(r, &nt);
        const int32_t       *te = str_er_result_text_ers(r, &ne);
        const str_er_gbound *gb = str_er_result_group_bounds(r, &nb);
        for (int32_t k = 0; k < nb; ++k) {
            ER *e = all_er[(size_t)k];
            e->bound.x = gb[k].x; e->bound.y = gb[k].y; e->bound.width = gb[k].w; e->bound.height = gb[k].h;
            e->center.x = gb[k].cx; e->center.y = gb[k].cy;
        }
        (void)ne;
        const ERs in(all_er);
        for (int32_t i = 0; i < nt; ++i) {
            Text t;
            for (int32_t k = 0; k < tx[i].count; ++k) t.ers.push_back(in[(size_t)te[tx[i].first + k]]);
            t.slope = tx[i].slope;
            t.box.x = tx[i].x; t.box.y = tx[i].y; t.box.width = tx[i].w; t.box.height = tx[i].h;
            text.push_back(t);
        }
        int32_t na = 0;
        const int32_t *ga = str_er_result_group_all(r, &na);       // all_er: sorted, inner-suppressed
        all_er.clear();
        for (int32_t k = 0; k < na; ++k) all_er.push_back(in[(size_t)ga[k]]);
    }

    // void ERFilter::er_delete(ER *er) (src/ER.cpp:194-233): the table owns the nodes
    void er_delete(ERTree &tree) { tree.nodes.clear(); tree.root = nullptr; }

    str_er_ctx *handle() const { return ctx_.get(); }

private:
    double MIN_OCR_PROB;
    std::shared_ptr<str_er_ctx> ctx_;

    void check(int rc) const
    {
        if (rc != STR_ER_OK) throw std::runtime_error(std::string(str_er_strerror(rc)) + ": " + str_er_last_error(ctx_.get()));
    }
    // the outputs of lattice_decode_words(_host) sized for the words: a run has at most 4 lattice parts
    static LatticeDecodes lattice_out(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                                      const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs)
    {
        if (first_run.size() != n_runs.size() || run_costs.size() != 65 * splits.size() || piece_costs.size() % 65)
            throw std::invalid_argument("lattice_decode_words: 65 bytes a run and a piece, one record a run, one span a word");
        size_t cap = 1;
        for (const int32_t k : n_runs) cap += 4 * (size_t)(k > 0 ? k : 0);
        if (cap > 0x7FFFFFFFull) throw std::invalid_argument("lattice_decode_words: too many runs");
        LatticeDecodes out;
        out.decodes.resize(first_run.size());
        out.chars.resize(64 * first_run.size());
        out.src.resize(64 * first_run.size());
        out.parts.resize(cap);
        return out;
    }
    // the outputs of lattice_decode_lines(_host) sized for the runs: 3 labels a node, a part a node at the most (one entry more than
    // needed, so that no pointer is null)
    static LineLatticeDecodes line_lattice_out(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                                               const std::vector<uint8_t> &gaps, const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs)
    {
        if (first_run.size() != n_runs.size() || run_costs.size() != 65 * splits.size() || gaps.size() != 2 * splits.size() || piece_costs.size() % 65)
            throw std::invalid_argument("lattice_decode_lines: 65 bytes a run and a piece, one record and one gap pair a run, one span a line");
        size_t atoms = 0;
        for (const str_er_run_split &S : splits) atoms += (size_t)(S.n_cuts < 0 ? 0 : S.n_cuts > 3 ? 3 : S.n_cuts) + 1;
        if (atoms > 0x7FFFFFFFull / 3) throw std::invalid_argument("lattice_decode_lines: too many runs");
        LineLatticeDecodes out;
        out.decodes.resize(first_run.size());
        out.chars.assign(3 * atoms + 1, 0xFF);
        out.src.assign(3 * atoms + 1, 0xFFFF);
        out.parts.resize(atoms + 1);
        out.word_of_part.assign(atoms + 1, -1);
        return out;
    }
    static void line_lattice_trim(LineLatticeDecodes &out, int32_t n_parts)
    {
        out.chars.pop_back(); out.src.pop_back();
        out.parts.resize((size_t)n_parts); out.word_of_part.resize((size_t)n_parts);
    }
    // the outputs of lattice_match_words(_host) sized for the words: a run has at most 4 parts
    static LatticeMatches lattice_match_out(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                                            const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs)
    {
        if (first_run.size() != n_runs.size() || run_costs.size() != 65 * splits.size() || piece_costs.size() % 65)
            throw std::invalid_argument("lattice_match_words: 65 bytes a run and a piece, one record a run, one span a word");
        size_t cap = 1;
        for (const int32_t k : n_runs) cap += 4 * (size_t)(k > 0 ? k : 0);
        if (cap > 0x7FFFFFFFull) throw std::invalid_argument("lattice_match_words: too many runs");
        LatticeMatches out;
        out.matches.resize(first_run.size());
        out.src.resize(32 * first_run.size());
        out.parts.resize(cap);
        return out;
    }
    // the outputs of lattice_match_tracks(_host) sized for the tracks: a usable member has at most 32 parts
    static LatticeTrackMatches lattice_track_out(const std::vector<str_er_run_split> &splits, const std::vector<uint8_t> &run_costs, const std::vector<uint8_t> &piece_costs,
                                                 const std::vector<int32_t> &first_run, const std::vector<int32_t> &n_runs, const std::vector<int32_t> &track_first,
                                                 const std::vector<int32_t> &track_count, const std::vector<int32_t> &members)
    {
        if (first_run.size() != n_runs.size() || run_costs.size() != 65 * splits.size() || piece_costs.size() % 65 || track_first.size() != track_count.size())
            throw std::invalid_argument("lattice_match_tracks: 65 bytes a run and a piece, one record a run, one span a word, one span a track");
        const size_t cap = 1 + 32 * members.size();
        if (cap > 0x7FFFFFFFull) throw std::invalid_argument("lattice_match_tracks: too many members");
        LatticeTrackMatches out;
        out.matches.resize(track_first.size());
        out.members.resize(members.size());
        out.src.resize(32 * members.size());
        out.parts.resize(cap);
        return out;
    }
    // the regions of er_masks / er_shapes / er_strokes: of every ER its bound, level and key
    static std::vector<str_er_cand> regions_of(const ERs &ers)
    {
        std::vector<str_er_cand> regions(ers.size());
        for (size_t i = 0; i < ers.size(); ++i) {
            str_er_cand &c = regions[i];
            c = str_er_cand{};
            c.x = (uint16_t)ers[i]->bound.x; c.y = (uint16_t)ers[i]->bound.y; c.w = (uint16_t)ers[i]->bound.width; c.h = (uint16_t)ers[i]->bound.height;
            c.level = (uint8_t)ers[i]->level; c.key = ers[i]->key;
        }
        return regions;
    }
    void load(int which, const std::string &file)
    {
        // the reference prints and returns false (src/adaboost.cpp:877-881); callers ignore it (src/main.cpp:23-24).
        check(str_er_load_cascade(ctx_.get(), which, file.c_str()));
    }

    // node table -> intrusive tree with the reference's parent/child/next links; children are
    // prepended like er_merge does (src/ER.cpp:183-185), in ascending key order overall.
    static void unpack_plane(const str_er_result *r, int plane, ERTree &tree, ERs &pool, ERs &strong, ERs &weak)
    {
        int32_t nn = 0, nc = 0;
        const str_er_node *nodes = str_er_result_plane_nodes(r, plane, &nn);
        const str_er_cand *cands = str_er_result_plane_cands(r, plane, &nc);
        str_er_plane_info info;
        str_er_result_plane_info(r, plane, &info);
        tree.nodes.assign((size_t)nn, ER());
        tree.root = nn ? &tree.nodes[info.root] : nullptr;
        for (int i = 0; i < nn; ++i) {
            ER &e = tree.nodes[i];
            const str_er_node &n = nodes[i];
            e.level = n.level; e.area = n.area; e.key = n.key; e.ch = info.ch;
            e.bound.x = n.x; e.bound.y = n.y; e.bound.width = n.w; e.bound.height = n.h;
            e.pixel = (int)n.key; e.x = (int)(n.key % (uint32_t)info.width); e.y = (int)(n.key / (uint32_t)info.width);
        }
        for (int i = nn - 1; i >= 0; --i) {       // descending index + prepend = ascending child lists
            if (i == info.root) continue;
            ER &e = tree.nodes[i];
            ER &p = tree.nodes[nodes[i].parent];
            e.parent = &p; e.next = p.child; p.child = &e;
        }
        for (int i = 0; i < nc; ++i) {
            const str_er_cand &c = cands[i];
            if (c.node < 0) continue;
            ER *e = &tree.nodes[c.node];
            e->score_strong = c.score_strong; e->score_weak = c.score_weak;
            pool.push_back(e);
            if (c.cls == STR_ER_CLS_STRONG) strong.push_back(e);
            else if (c.cls == STR_ER_CLS_WEAK) weak.push_back(e);
        }
    }
};

// `class OCR` of the reference (inc/OCR.h:26-53), the part on the config-3 path: the constructor loads the
// libsvm model (OCR::OCR, src/OCR.cpp:19-22) and chain_run scores one ER (src/OCR.cpp:67-140).  It shares the
// ERFilter's context (the reference hangs the OCR object off ERFilter::ocr, inc/ER.h:119).
class OCR {
public:
    OCR(ERFilter &filter, const char *svm_file_name, int _img_L = 30, int _feature_L = 15) : ctx_(filter.handle())
    {
        if (_img_L != 30 || _feature_L != 15) throw std::runtime_error("OCR: only img_L = 30, feature_L = 15 (src/main.cpp:25) are built");
        if (str_er_load_svm_model(ctx_, svm_file_name, 8 * _feature_L * _feature_L) != STR_ER_OK)
            throw std::runtime_error(std::string("svm_load_model: ") + str_er_last_error(ctx_));
    }

    // double OCR::chain_run(Mat src, int thresh, double slope): src = channel(bound).  Returns table[label] + prob.
    // `thresh` is ignored exactly as in the reference (THRESH_OTSU overrides it); |slope| > 0.01 rotates the
    // binarised ROI by atan2(slope, 1) first (rotate_mat, src/OCR.cpp:73-78).
    double chain_run(const Image8 &plane, const Rect &bound, int /*thresh*/, double slope)
    {
        const int32_t box[4] = {bound.x, bound.y, bound.width, bound.height};
        int32_t label = 0;
        double  prob = 0;
        const int rc = str_er_ocr_chain_run_slope(ctx_, plane.data, plane.cols, plane.rows, plane.step, box, &slope, 1, &label, &prob, nullptr);
        if (rc != STR_ER_OK) throw std::runtime_error(std::string("chain_run: ") + str_er_last_error(ctx_));
        static const char *table = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz&()";   // src/OCR.cpp:10
        return (label >= 0 && label < 65 ? table[label] : '?') + prob;
    }

private:
    str_er_ctx *ctx_;
};

} // namespace str_er_host
