// er_kernels.h -- host-callable launchers of the gfx950 kernels in er_kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include "er_types.h"

namespace str_er {

struct BatchDev {
    const PlaneDesc *planes;   // device array [n_planes]
    PlaneCtr        *ctr;      // device array [n_planes]
    int32_t          n_planes;
    uint32_t         n_tiles;  // batch-wide
    uint32_t         n_pairs;  // batch-wide seam pixel pairs
    uint32_t         n_node_blocks; // workgroups of the per-record kernels, batch-wide
    const uint16_t  *nb_plane;   // plane of every such workgroup (a plane has PlaneDesc::nb_count of them, from nb_base on)
    NodeArrays       na;
    KeptArrays       ka;
    const uint16_t  *tile_plane;        // plane of every tile
    const uint16_t  *seam_block_plane;  // plane of every k_seam workgroup
    const uint32_t  *seam_block_first;  // its first pair inside that plane
    uint32_t         n_seam_blocks;
    uint32_t        *tile_nbase; // plane-local id of every tile's first node record (NONE: the plane ran out of records)
    uint16_t        *tile_nrec;  // ... and how many records the tile has
    uint8_t         *group_done; // per group of tiles: k_group_merge has joined its inner seams
    uint32_t        *undone_list, *undone_count;    // the groups k_group_merge left alone (too many records): their inner seams are joined by k_seam_undone
    uint32_t        *bin_list, *bin_count;          // k_group_bins: the groups by the table that holds their records (list k at bin_list + k * n_groups, bin_count[k] long; bin_count[4]: one-tile groups)
    const uint16_t  *group_plane; // plane of every group
    uint32_t         n_groups;   // batch-wide
    int32_t          group_x, group_y;   // tiles per group (0: no grouping in this batch)
    uint16_t        *seam;     // node of every tile-border pixel: index inside its tile's records (0xFFFF: wall)
    uint32_t        *pool;     // kept slots chosen by NMS, ascending key
    uint32_t        *pool_tmp;
    CandRec         *cands;    // packed, ordered by (plane, key)
    uint32_t        *total_cands;
    uint16_t        *cand_plane; // plane of every packed candidate
    uint32_t        *watch;      // [n_planes x NMS_WATCH_CAP] key pixels of the children that may compete for a parent
    uint32_t        *wstamp;     // ... and, after the flood order walk, their stamps (order of first access; 0xFFFFFFFF: later than all stamped ones)
    uint32_t        *wparent;    // ... and the kept slot of the parent each one may compete for (the walk stops once every parent's order is decided)
};

// compute_channels (src/ER.cpp:114-128): interleaved BGR -> Y, Cr, Cb planes.
void launch_bgr_to_ycrcb(hipStream_t s, const uint8_t *bgr, int w, int h, int64_t stride,
                         int64_t frame_pitch, int n_frames, uint8_t *y, uint8_t *cr, uint8_t *cb,
                         int dstride, int64_t dst_frame_pitch);
// NV12 (luma plane, then interleaved Cb/Cr at half resolution, same row stride) -> the same three planes; chroma replicated 2 x 2
void launch_nv12_to_ycrcb(hipStream_t s, const uint8_t *nv12, int w, int h, int64_t stride, int64_t frame_pitch, int n_frames, uint8_t *y, uint8_t *cr,
                          uint8_t *cb, int dstride, int64_t dst_frame_pitch);
// 255 - x for the single-stage compute_channels entry point.
void launch_invert(hipStream_t s, const uint8_t *src, uint8_t *dst, size_t n);
// cv::resize INTER_LINEAR 8UC1 semantics; z planes with the given pitches.
void launch_resize(hipStream_t s, const uint8_t *src, int sw, int sh, int sstride, int64_t splane_pitch,
                   int64_t sframe_pitch, uint8_t *dst, int dw, int dh, int dstride, int64_t dplane_pitch,
                   int64_t dframe_pitch, int planes_per_frame, int n_frames);
// A pyramid level: k_pyr_level where the shape qualifies (linear, 1 < scale <= 1.5 both ways, everything dword-aligned, `enable`), launch_resize otherwise.
// rows: output rows a wave walks (8 / 16 / 32; 0: the kernel's own choice, 8).  Returns the rows k_pyr_level ran with, 0 when k_resize ran.
int  launch_pyr_level(hipStream_t s, const uint8_t *src, int sw, int sh, int sstride, int64_t splane_pitch, int64_t sframe_pitch, uint8_t *dst, int dw, int dh,
                      int dstride, int64_t dplane_pitch, int64_t dframe_pitch, int planes_per_frame, int n_frames, int rows, bool enable);

// Lists of frames of different sizes (str_er_detect_bgr_list / _nv12_list): a job is one frame (ingest) or one frame's pyramid level (resize, `planes`
// planes per job).  The kernels' device table -- *_table_bytes(n) bytes -- is built on the host into `out` and copied to the device by
// the caller; the builders return the workgroups of the launch.  One launch for all jobs.
struct IngestJob {
    const uint8_t *src; int64_t stride;           // BGR frame (device memory); NV12: its luma plane, chroma h rows further on
    uint8_t *dst; int64_t plane_pitch;            // its Y plane; Cr and Cb follow plane_pitch bytes apart
    int32_t w, h, dstride;
};
struct ResizeJob {
    const uint8_t *src; uint8_t *dst; int64_t splane_pitch, dplane_pitch;     // first source / destination plane, the others that far apart
    int32_t sw, sh, sstride, dw, dh, dstride;
};
size_t   ingest_table_bytes(int n);
size_t   resize_table_bytes(int n);
uint32_t build_ingest_table(const IngestJob *jobs, int n, void *out);
uint32_t build_resize_table(const ResizeJob *jobs, int n, int planes, void *out);
void     launch_bgr_to_ycrcb_list(hipStream_t s, const void *d_table, int n, uint32_t n_wg);
void     launch_nv12_to_ycrcb_list(hipStream_t s, const void *d_table, int n, uint32_t n_wg);
void     launch_resize_list(hipStream_t s, const void *d_table, int n, uint32_t n_wg);

// sparse: the small-LDS / high-occupancy size of the kernel (text-like frames); dense: the big one (noise-like frames)
// list: the tiles to work on (batch-wide tile numbers, device), nullptr = all tiles of the batch
void launch_tile_tree(hipStream_t s, const BatchDev &b, const DetectParams &p, bool sparse, const uint32_t *list = nullptr, uint32_t n = 0);
// the tiles k_tile_tree2 handed back (list / count on the device): `grid` workgroups walk the list
void launch_tile_tree_fb(hipStream_t s, const BatchDev &b, const DetectParams &p, bool sparse, const uint32_t *list, const uint32_t *count, uint32_t grid);
// k_tile_tree2 (er_tile_tree2.inl): the level-by-level / bit-mask form for planes with few levels per tile; one wave per pair of horizontally
// adjacent tiles (entry: first tile | 1 << 31 if the tile to its right takes part); tiles it does not take end up in fb_list
void launch_tile_tree2(hipStream_t s, const BatchDev &b, const DetectParams &p, const uint32_t *pairs, uint32_t n_pairs, uint32_t *fb_list, uint32_t *fb_count);
// the tiles of every group of BatchDev::group_x x group_y tiles joined in LDS, in place (variant: LDS capacity / lanes, see er_kernels.hip)
void launch_group_merge(hipStream_t s, const BatchDev &b, int variant, const uint32_t *glist = nullptr, uint32_t n = 0);
// the groups sorted by their record count into the lists of four tables of caps[k] records (BatchDev::bin_list / bin_count), the rest onto the undone list;
// then per table k (512 / 1024 / 2048 / 2528 records) `grid` workgroups walk its list
void launch_group_bins(hipStream_t s, const BatchDev &b, const uint32_t caps[4]);
void launch_group_merge_list(hipStream_t s, const BatchDev &b, int k, uint32_t grid);
void launch_seam(hipStream_t s, const BatchDev &b, bool xcd_affine);
void launch_resolve(hipStream_t s, const BatchDev &b);
// strips of a plane extracted elsewhere: make a strip's record ids plane-wide; join pixel pairs (plane-local ids) across a cut
void launch_rebase_records(hipStream_t s, NodeRec *rec, uint32_t *aux, uint32_t n, uint32_t delta, uint32_t key_add, uint32_t y_add, uint32_t w, uint32_t h,
                           uint32_t *bad);
void launch_check_forest(hipStream_t s, NodeRec *plane_rec, uint32_t n, uint32_t *bad);
void launch_connect_cut(hipStream_t s, NodeRec *plane_rec, const uint32_t *bot, const uint32_t *top, uint32_t w, uint32_t base_lo, uint32_t n_lo, uint32_t base_hi,
                        uint32_t n_hi, uint32_t *bad);
void launch_strip_border_ids(hipStream_t s, const uint16_t *seam_row, const uint32_t *tile_nbase_row, int w, uint32_t *out);
// er_merge's accumulation (src/ER.cpp:153-165) for the whole batch in ONE launch: a node pushes its totals to its parent when its
// last open child has pushed (dependency counters, agent-scope release/acquire)
void launch_reduce(hipStream_t s, const BatchDev &b);
void launch_root(hipStream_t s, const BatchDev &b, const DetectParams &p);
void launch_select(hipStream_t s, const BatchDev &b, const DetectParams &p);
void launch_kept(hipStream_t s, const BatchDev &b, const DetectParams &p);
// pass 0: every plane; sibling ties by key (exact mode: provisional, planes with ties are counted in n_amb and get a watch list).
// use_index_order: exact mode on an uploaded tree -- the table order is the child-list order.
void launch_nms(hipStream_t s, const BatchDev &b, const DetectParams &p, bool use_index_order = false);
void launch_nms_alt(hipStream_t s, const BatchDev &b, const DetectParams &p, uint32_t *alt_list /* NMS_ALT_CAP words, device */);
// planes with ties left (PlaneCtr::n_rel) -> host-addressable memory: pixels, watch keys, watch parents per slot (see er_kernels.hip)
void launch_export_listed_planes(hipStream_t s, const BatchDev &b, const ReplayItem *items, int n_items, uint8_t *host_buf /* page-locked, device-addressable */);
void launch_export_tie_planes(hipStream_t s, const BatchDev &b, uint8_t *host_buf, size_t slot_bytes, int n_slots, uint32_t *slot_plane_dev /* n_slots words, device */,
                              uint32_t *count, uint32_t *slot_plane);
// exact mode, planes with sibling ties: replay the reference's flood (src/ER.cpp:240-374) to stamp every pixel with the order in
// which it becomes accessible, then NMS again with the ties decided by those stamps.  scratch: see ReplayItem.
size_t replay_scratch_bytes(int w, int h);
void launch_flood_order(hipStream_t s, const BatchDev &b, const DetectParams &p, const ReplayItem *items, int n_items, uint8_t *scratch);
void launch_nms_resolve(hipStream_t s, const BatchDev &b, const DetectParams &p, const ReplayItem *items, int n_items, const uint8_t *scratch);
void launch_cand_prefix(hipStream_t s, const BatchDev &b);
// classify (src/ER.cpp:507-528) over the packed pool of the batch.
void launch_classify(hipStream_t s, const BatchDev &b, const DetectParams &p, CascadeDev strong,
                     CascadeDev weak, int run_cascades, const uint32_t *list = nullptr, const uint32_t *n_list = nullptr, bool few = false,
                     uint32_t hint = 0, int force_grid = 0, int form = 0);      // (few: a call of a frame or two -- 16 candidates on 16 waves instead of 32 on 4; hint: the previous batch's candidates, for the grid)
// after the NMS tie pass: new candidate offsets (b.cands / b.cand_plane = the second set of buffers), the records of unchanged planes
// moved over from `from`, the candidates of the changed planes listed in redo[0 .. *n_redo) for launch_classify
// (calls of a frame or two) the counter block and the first candidate records to device-addressable host memory, one launch
void launch_results_to_host(hipStream_t s, const void *ctr_block, void *to_ctr, size_t ctr_bytes, const CandRec *cands, CandRec *to_cands, uint32_t cap_cands,
                            const uint32_t *total_cands);
void launch_cand_reprefix(hipStream_t s, const BatchDev &b, const CandRec *from, uint32_t *redo, uint32_t *n_redo);

// Stand-alone classify chain on explicit boxes of one device plane (single-stage API).
void launch_lbp_boxes(hipStream_t s, const uint8_t *plane, int w, int h, int stride, const int32_t *boxes,
                      int n, double *hist /*n*1024 or null*/, uint8_t *tiles /*n*676 or null*/, uint8_t *codes /*n*576 or null*/, uint8_t *cls,
                      double *s_strong, double *s_weak, CascadeDev strong, CascadeDev weak, int run_cascades);

// CascadeBoost::predict on explicit feature vectors (n x 1024 doubles).
void launch_cascade_fv(hipStream_t s, const double *fv, int n, double *out, CascadeDev c);

// Pixel masks of regions (er_masks.inl).  The jobs come ordered by size class (mask_class: 0 registers, 1 LDS, 2 global scratch),
// n_class[k] of class k; out receives the bit rows at MaskJob::out_off, pixels[MaskJob::idx] the popcounts.  scratch: the
// mask_scratch_words of every class-2 job, at its MaskJob::scratch_off (may be null without class-2 jobs).  shapes != null: also
// shapes[MaskJob::idx] receives the mask's ShapeRec (the SHAPES instantiations); strokes != null: strokes[MaskJob::idx] its StrokeRec
// (the STROKES instantiations); both null run the mask kernels alone.
int    mask_class(int w, int h);
size_t mask_scratch_words(int w, int h);
void   launch_er_masks(hipStream_t s, const MaskJob *jobs, const int n_class[3], uint32_t *out, uint32_t *pixels, ShapeRec *shapes, StrokeRec *strokes,
                       uint64_t *scratch, float qscale);

// Line crops (er_line_crops.inl): n jobs, one workgroup each.  out receives the grey crops at LineCropJob::out_off; with glyph != null
// also the glyph crops (same offsets), from the members and the mask words `bits` they index.
void launch_line_crops(hipStream_t s, const LineCropJob *jobs, int n, uint8_t *out, uint8_t *glyph, const GlyphMember *members, const uint32_t *bits);

// Text maps (er_text_map.inl): one wave per tile.  map (or null) receives the OR of the values, ids (or null) the smallest id or -1, of
// the regions of every tile that cover each element; tabs holds the uint16 xs / ys tables the regions index; bits the mask words.
void launch_text_map(hipStream_t s, const TextMapTile *tiles, int n_tiles, const uint32_t *list, const TextMapCand *cands, const uint16_t *tabs,
                     const uint32_t *bits, uint8_t *map, int32_t *ids);

// Frame lines (er_frame_lines.inl).  launch_line_foot: one wave per job; feet receives the footprint rows of every line at
// FootLine::word_off, stat[line] (zeroed by the caller) the pixels and the extent of the set bits; members / tabs / bits as for the
// text maps.  launch_foot_pairs: one wave per line over the later lines of its frame (list); the pairs with a common pixel go to
// out[0 .. cap), head (zeroed by the caller) counts them -- also those past cap -- and the pairs whose boxes intersect.
void launch_line_foot(hipStream_t s, const FootJob *jobs, int n_jobs, const FootLine *lines, const TextMapCand *members, const uint16_t *tabs,
                      const uint32_t *bits, uint64_t *feet, FootStat *stat);
void launch_foot_pairs(hipStream_t s, const FootLine *lines, int n_lines, const uint32_t *list, const uint64_t *feet, FootHead *head, FootPair *out,
                       uint32_t cap);
// launch_foot_links (STR_ER_WANT_LINE_LINKS, str_er_link_feet): one wave per line a over list[range[a].first .. range[a].end), the lines
// of the next adjacent frame; out / head as for launch_foot_pairs (a table and a head of their own)
void launch_foot_links(hipStream_t s, const FootLine *lines, int n_lines, const FootRange *range, const uint32_t *list, const uint64_t *feet, FootHead *head,
                       FootPair *out, uint32_t cap);
// launch_foot_geom (STR_ER_WANT_LINE_GEOM, str_er_feet_geom): one wave per line over its footprint in feet: the moments and the number
// of hull vertices into recs[line], the vertices (absolute x, y pairs, in the order of str_er_line_geom) into xy from slots[line].pt_first
// on; scratch: h + 1 words from slots[line].x_first on for every line with h + 1 > GEOM_LDS_ROWS (may be null when there is none)
void launch_foot_geom(hipStream_t s, const FootLine *lines, int n_lines, const GeomSlot *slots, const uint64_t *feet, uint64_t *scratch, GeomRec *recs,
                      int32_t *xy);
// launch_foot_words (STR_ER_WANT_LINE_WORDS, str_er_feet_words): one wave per line over its footprint in feet: the number of glyph runs
// and colmax into recs[line], the runs (frame columns and rows, ordered by column, word = -1) into runs from slots[line].first on, at
// most slots[line].cap of them.  Every line must be at most WORDS_MAX_BOX wide and tall (a larger one is left without runs)
void launch_foot_words(hipStream_t s, const FootLine *lines, int n_lines, const WordsSlot *slots, const uint64_t *feet, WordsRec *recs, WordsRun *runs);
// launch_run_tiles (STR_ER_WANT_RUN_READ, str_er_feet_read): the byte tile of every run of tiles (0 where the footprint has the pixel,
// else 255; the contract is at str_er_run_read) from the footprint words in feet into atlas, whose rows are stride bytes (a multiple
// of 4; atlas aligned to 4).  A tile's rows and columns must lie inside its line's footprint and its place inside the atlas
// (pack_run_tiles): the host checks both before the launch
void launch_run_tiles(hipStream_t s, const RunTile *tiles, int n_tiles, const uint64_t *feet, uint8_t *atlas, uint32_t stride);

} // namespace str_er
