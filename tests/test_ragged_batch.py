"""Frames of different sizes in one call (str_er_detect_bgr_list / str_er_detect_planes_list): every plane against the oracle,
every record against one call per frame, device frames, sibling ties, the layout cache, and the errors."""
import gzip
import os

import numpy as np
import pytest

from conftest import check_plane_against_oracle

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _crops():
    z = np.load(os.path.join(GOLDEN, "icdar_crops.npz"))
    return [np.ascontiguousarray(z[k]) for k in sorted(z.files)]


def _ctx(S, cascade_paths, **kw):
    f = S.ERFilter(params=S.Params(**kw))
    f.load_cascade(0, cascade_paths[0])
    f.load_cascade(1, cascade_paths[1])
    return f


def _planes_of(res, i):
    return [p for p in res.planes if p.frame == i]


def test_mixed_sizes_match_the_oracle(S, cascade_paths, oracle, oracle_cascades):
    f = _ctx(S, cascade_paths, max_width=1920, max_height=1080, max_frames=8)
    sy = S.synth
    frames = _crops() + [sy.stext_bgr(sy.frame_seed(3), 1920, 1080), sy.stext_bgr(sy.frame_seed(4), 641, 359),
                         sy.snoise_bgr(sy.frame_seed(5), 200, 100), sy.stext_bgr(sy.frame_seed(6), 1, 1)]
    assert len(frames) == 8
    res = f.text_detect_list(frames, want_nodes=True)
    assert len(res.planes) == 6 * len(frames)
    for i, fr in enumerate(frames):
        ps = _planes_of(res, i)
        assert [p.ch for p in ps] == list(range(6))
        six = oracle.compute_channels(fr)
        for p in ps:
            assert (p.width, p.height) == (fr.shape[1], fr.shape[0])
            check_plane_against_oracle(oracle, p, six[p.ch], oracle_cascades)
    f.close()


def _renumber_check(one, lst, i):
    """Frame i of the list result `lst` against `one` (that frame alone): byte-identical records, indices shifted."""
    sel = np.nonzero(lst.cands["frame"] == i)[0]
    co = int(sel[0]) if len(sel) else 0
    assert len(sel) == len(one.cands) and (len(sel) == 0 or (sel == np.arange(co, co + len(sel))).all())
    pinfo = lst.info[lst.info["frame"] == i]
    poff = int(np.nonzero(lst.info["frame"] == i)[0][0])
    exp = one.info.copy()
    exp["frame"] = i
    assert pinfo.tobytes() == exp.tobytes()
    got = lst.cands[sel].copy()
    assert (got["plane"] >= poff).all()
    got["plane"] -= poff
    exp = one.cands.copy()
    exp["frame"] = i
    assert got.tobytes() == exp.tobytes()
    for k in range(len(one.info)):
        a, b = one.planes[k].nodes, lst.planes[poff + k].nodes
        assert a.tobytes() == b.tobytes()
    if one.ocr_label is not None:
        assert lst.ocr_label[sel].tobytes() == one.ocr_label.tobytes() and lst.ocr_prob[sel].tobytes() == one.ocr_prob.tobytes()
    assert lst.tracks[sel].tobytes() == one.tracks.tobytes()
    assert lst.group_bounds[sel].tobytes() == one.group_bounds.tobytes()
    # texts of the frame: a contiguous run; their members are candidate indices, images concatenated
    tsel = np.nonzero(lst.texts["frame"] == i)[0]
    assert len(tsel) == len(one.texts)
    t = lst.texts[tsel].copy()
    m0 = int(t["first"][0]) if len(t) else 0
    t["frame"] = 0
    t["first"] -= m0
    assert t.tobytes() == one.texts.tobytes()
    n_m = len(one.text_ers)
    assert (lst.text_ers[m0:m0 + n_m] - co).tobytes() == one.text_ers.tobytes()
    ga = lst.group_all[(lst.group_all >= co) & (lst.group_all < co + len(sel))] - co
    assert ga.tobytes() == one.group_all.tobytes()
    if one.line_label is not None:
        assert lst.line_label[m0:m0 + n_m].tobytes() == one.line_label.tobytes()
        assert lst.line_prob[m0:m0 + n_m].tobytes() == one.line_prob.tobytes()
        assert lst.line_kept[m0:m0 + n_m].tobytes() == one.line_kept.tobytes()
        assert lst.text_alive[tsel].tobytes() == one.text_alive.tobytes()


def test_list_equals_one_call_per_frame(S, cascade_paths, oracle, oracle_cascades):
    W, H, L = 1024, 768, 8
    f = _ctx(S, cascade_paths, max_width=W, max_height=H, max_frames=6, n_pyr_levels=L, channel_mask=0x07)
    f.load_svm_model_text(gzip.open(S.cascade_io.ocr_model_path()).read(), 1800)
    sy = S.synth
    frames = [sy.stext_bgr(sy.frame_seed(11), 1024, 768), _crops()[0], sy.stext_bgr(sy.frame_seed(12), 641, 359),
              sy.stext_bgr(sy.frame_seed(13), 333, 517), sy.stext_bgr(sy.frame_seed(14), 1000, 200)]
    st = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP | S.STAGE_OCR | S.STAGE_OCR_LINES
    lst = f.text_detect_list(frames, st, want_nodes=True)
    assert lst.texts is not None and len(lst.texts) > 0
    for i, fr in enumerate(frames):
        ps = _planes_of(lst, i)
        assert [(p.width, p.height) for p in ps] == \
            [oracle.pyr_dims(fr.shape[1], fr.shape[0], l) for l in range(L) for _ in range(3)]
        one = f.text_detect(fr, st, want_nodes=True)
        _renumber_check(one, lst, i)
    for i in (1, 3):         # the pyramid itself, through the oracle
        six = oracle.compute_channels(frames[i])
        pyr = {c: oracle.pyramid(six[c], L) for c in range(3)}
        for p in _planes_of(lst, i):
            check_plane_against_oracle(oracle, p, pyr[p.ch][p.pyr], oracle_cascades)
    f.close()


_DEVICE_CHILD = r"""
import sys
import numpy as np
import torch                                    # (first: the HIP runtime PyTorch brings, as in smoke())
sys.path.insert(0, sys.argv[1])
import importlib
S = importlib.import_module("scene-text-recognition_amd")
f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=4))
f.load_cascade(0, sys.argv[2]); f.load_cascade(1, sys.argv[3])
sy = S.synth
crop = np.ascontiguousarray(np.load(sys.argv[4])["{crop}"])
frames = [sy.stext_bgr(sy.frame_seed(21), 640, 480), sy.stext_bgr(sy.frame_seed(22), 321, 243), sy.snoise_bgr(sy.frame_seed(23), 97, 61), crop]
host = f.text_detect_list(frames, want_nodes=True)
bufs, refs = [], []
for k, fr in enumerate(frames):
    h, w, _ = fr.shape
    pitch = 3 * w + 7 + 2 * k                   # odd row pitches, and the frame starts 1 + k bytes into its buffer
    buf = np.zeros(1 + k + pitch * h, np.uint8)
    for y in range(h):
        buf[1 + k + y * pitch:1 + k + y * pitch + 3 * w] = fr[y].reshape(-1)
    t = torch.from_numpy(buf).cuda()
    bufs.append(t)
    refs.append((t.data_ptr() + 1 + k, w, h, pitch))
torch.cuda.synchronize()
dev = f.detect_bgr_list_device(refs, S.STAGE_ALL | S.WANT_NODES)
assert dev.info.tobytes() == host.info.tobytes() and dev.cands.tobytes() == host.cands.tobytes()
for a, b in zip(dev.planes, host.planes):
    assert a.nodes.tobytes() == b.nodes.tobytes()
big = np.zeros((480 + 5, 640 + 9, 3), np.uint8)     # host views with a row stride (no copy) give the same
big[2:2 + 243, 3:3 + 321] = frames[1]
view = f.text_detect_list([frames[0], big[2:2 + 243, 3:3 + 321], frames[2], frames[3]], want_nodes=True)
assert view.cands.tobytes() == host.cands.tobytes()
print("device list == host list:", len(host.cands), "candidates")
"""


def test_device_frames_at_odd_pitches(S, cascade_paths):
    """Frames in device memory (torch tensors) at odd pitches and unaligned starts == the same frames from the host.  In a child
    process that loads PyTorch's HIP runtime before the library, as smoke() does (this process has the library's own by now)."""
    import subprocess
    import sys
    z = np.load(os.path.join(GOLDEN, "icdar_crops.npz"))
    code = _DEVICE_CHILD.replace("{crop}", sorted(z.files)[2])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, root, cascade_paths[0], cascade_paths[1], os.path.join(GOLDEN, "icdar_crops.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "device list == host list" in r.stdout


def _same_result(a, b, what):
    assert a.info.tobytes() == b.info.tobytes(), what + ": plane infos"
    assert a.cands.tobytes() == b.cands.tobytes(), what + ": cands"
    assert len(a.planes) == len(b.planes) > 0
    for k, (x, y) in enumerate(zip(a.planes, b.planes)):
        assert x.nodes.tobytes() == y.nodes.tobytes(), "%s: nodes of plane %d" % (what, k)


def test_equal_frames_uniform_and_list_front_ends_agree(S, cascade_paths):
    """Frames of one size through the uniform front end and through the list front end: byte-identical plane infos, candidates and nodes.
    211 x 97 (212 x 98 for NV12): odd sizes, so every level's rows are padded and end in a row tail, and level 1 (x 2^-1/2) is 149 x 69 -- a
    layout of the planes that differs between the two front ends shows as a frame read at the wrong address.  The uniform call from
    a host cube at a row stride and a frame pitch that are not tight, and from the same bytes in device memory; the per-plane calls;
    a plane subset (level 0 only) against the level-0 planes of the full call."""
    import ctypes as C
    W, H, N, L = 211, 97, 3, 2
    f = _ctx(S, cascade_paths, max_width=224, max_height=112, max_frames=N, n_pyr_levels=L)
    sy = S.synth
    d_cube = C.c_void_p()
    # (device memory from the HIP runtime the library itself is linked with, found through the library's handle: PyTorch's would be a
    # second runtime in this process)
    hip_malloc, hip_memcpy, hip_free = f.L.hipMalloc, f.L.hipMemcpy, f.L.hipFree
    hip_malloc.argtypes, hip_memcpy.argtypes, hip_free.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    try:
        frames = [sy.stext_bgr(sy.frame_seed(90 + k), W, H) for k in range(N)]
        assert all(fr.shape == (H, W, 3) for fr in frames) and len({fr.tobytes() for fr in frames}) == 3
        lst = f.text_detect_list(frames, want_nodes=True)
        assert [(p.frame, p.pyr, p.ch) for p in lst.planes] == [(k, l, c) for k in range(N) for l in range(L) for c in range(6)]
        assert [(p.width, p.height) for p in lst.planes[6:12]] == [(149, 69)] * 6 and len(lst.cands) > 0
        # the uniform call: a host cube with 11 bytes between rows and 13 more between frames, filled with 0xA5 around the pixels
        stride = 3 * W + 11
        pitch = stride * H + 13
        cube = np.full(N * pitch, 0xA5, np.uint8)
        for k, fr in enumerate(frames):
            for y in range(H):
                cube[k * pitch + y * stride:k * pitch + y * stride + 3 * W] = fr[y].reshape(-1)
        rh = C.c_void_p()
        f._check(f.L.str_er_detect_bgr(f.h, cube.ctypes.data, W, H, stride, pitch, N, 0, S.STAGE_ALL | S.WANT_NODES, C.byref(rh)))      # (0: STR_ER_MEM_HOST)
        _same_result(f._collect(rh), lst, "uniform host cube (stride %d, pitch %d) against the list" % (stride, pitch))
        # ... the same bytes on the device
        assert hip_malloc(C.byref(d_cube), cube.size) == 0
        assert hip_memcpy(d_cube, cube.ctypes.data, cube.size, 1) == 0          # (hipMemcpyHostToDevice)
        dev = f.detect_bgr_device(d_cube.value, W, H, N, S.STAGE_ALL | S.WANT_NODES, stride=stride, frame_pitch=pitch)
        _same_result(dev, lst, "uniform device cube against the list")
        # the tight host batch, as text_detect passes it
        full = f.text_detect(np.stack(frames), want_nodes=True)
        _same_result(full, lst, "text_detect against text_detect_list")
        # NV12
        nv = [sy.nv12_from_bgr(sy.stext_bgr(sy.frame_seed(93 + k), W + 1, H + 1)) for k in range(N)]
        assert all(a.shape == ((H + 1) * 3 // 2, W + 1) for a in nv)
        nv_lst = f.text_detect_nv12_list(nv, want_nodes=True)
        assert len(nv_lst.planes) == N * L * 6 and len(nv_lst.cands) > 0
        _same_result(f.text_detect_nv12(np.stack(nv), W + 1, H + 1, want_nodes=True), nv_lst, "text_detect_nv12 against text_detect_nv12_list")
        # the per-plane calls
        planes = [sy.gray(fr) for fr in frames]
        pl_lst = f.detect_planes_list(planes, want_nodes=True)
        assert [(p.width, p.height, p.ch) for p in pl_lst.planes] == [(W, H, k) for k in range(N)]
        _same_result(f.detect_planes(np.stack(planes), want_nodes=True), pl_lst, "detect_planes against detect_planes_list")
        # a plane subset: level 0 only (the pyramid is not built), exactly the level-0 planes of the full call
        sub = f.text_detect_planes(np.stack(frames), [1] * 6 + [0] * 6, want_nodes=True)
        keep = np.nonzero(full.info["pyr"] == 0)[0]
        assert len(keep) == N * 6 and sub.info.tobytes() == full.info[keep].tobytes()
        exp = full.cands[np.isin(full.cands["plane"], keep)].copy()
        exp["plane"] = np.searchsorted(keep, exp["plane"])
        assert len(exp) > 0 and sub.cands.tobytes() == exp.tobytes()
        for k, j in enumerate(keep):
            assert sub.planes[k].nodes.tobytes() == full.planes[j].nodes.tobytes()
    finally:
        if d_cube.value:
            hip_free(d_cube)
        f.close()


def test_sibling_ties_in_a_list(S, cascade_paths, oracle, oracle_cascades):
    f = _ctx(S, cascade_paths, max_width=480, max_height=360, max_frames=2, sibling_order=0)
    sy = S.synth
    frames = [sy.sties_bgr(sy.frame_seed(30), 480, 360, every=1), sy.sties_bgr(sy.frame_seed(31), 300, 220, every=1)]
    res = f.text_detect_list(frames, want_nodes=True)
    n_amb = 0
    for i, fr in enumerate(frames):
        six = oracle.compute_channels(fr)
        for p in _planes_of(res, i):
            check_plane_against_oracle(oracle, p, six[p.ch], oracle_cascades)
            n_amb += p.ambiguous
    assert n_amb > 0, "the tie frames made no NMS sibling tie"
    f.close()


def test_layout_cache_survives_list_calls(S, cascade_paths):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=3, n_pyr_levels=3, channel_mask=0x3F)
    sy = S.synth
    uni = np.stack([sy.stext_bgr(sy.frame_seed(40 + k), 640, 480) for k in range(3)])
    a = f.text_detect(uni, want_nodes=True)
    mixed = [sy.stext_bgr(sy.frame_seed(50), 200, 150), sy.stext_bgr(sy.frame_seed(51), 640, 480), sy.stext_bgr(sy.frame_seed(52), 77, 333)]
    m1 = f.text_detect_list(mixed, want_nodes=True)
    b = f.text_detect(uni, want_nodes=True)
    m2 = f.text_detect_list(mixed[::-1], want_nodes=True)
    c = f.text_detect(uni, want_nodes=True)
    for r in (b, c):
        assert r.info.tobytes() == a.info.tobytes() and r.cands.tobytes() == a.cands.tobytes()
        assert all(x.nodes.tobytes() == y.nodes.tobytes() for x, y in zip(r.planes, a.planes))
    # the list calls: each frame as it comes alone
    for i in range(3):
        one = f.text_detect(mixed[i], want_nodes=True)
        for lst, j in ((m1, i), (m2, 2 - i)):
            got = lst.cands[lst.cands["frame"] == j]
            fields = ["ch", "pyr", "key", "level", "cls", "area", "x", "y", "w", "h", "score_strong", "score_weak"]
            assert got[fields].tolist() == one.cands[fields].tolist()
    f.close()


def test_planes_list_matches_the_oracle(S, cascade_paths, oracle, oracle_cascades):
    f = _ctx(S, cascade_paths, max_width=640, max_height=480, max_frames=1)
    sy = S.synth
    planes = [sy.gray(sy.stext_bgr(sy.frame_seed(60), 640, 480)), sy.gray(_crops()[1]), sy.gray(sy.stext_bgr(sy.frame_seed(61), 123, 457)),
              sy.gray(sy.snoise_bgr(sy.frame_seed(62), 64, 32)), np.full((1, 1), 9, np.uint8),
              sy.gray(sy.stext_bgr(sy.frame_seed(63), 300, 200))[7:170, 5:290]]       # (a view with a row stride)
    res = f.detect_planes_list(planes, want_nodes=True)
    assert [p.ch for p in res.planes] == list(range(len(planes)))
    for p, img in zip(res.planes, planes):
        assert (p.width, p.height) == (img.shape[1], img.shape[0])
        check_plane_against_oracle(oracle, p, np.ascontiguousarray(img), oracle_cascades)
    f.close()


def test_list_errors_leave_the_context_usable(S, cascade_paths):
    import ctypes as C
    f = _ctx(S, cascade_paths, max_width=320, max_height=240, max_frames=2)
    L = f.L
    fr = S.synth.stext_bgr(S.synth.frame_seed(70), 320, 240)
    good = f.text_detect_list([fr])
    R = S.ImageRef

    def call(refs, n, mem):
        arr = (R * max(1, len(refs)))(*refs)
        rh = C.c_void_p()
        rc = L.str_er_detect_bgr_list(f.h, arr, len(refs) if n is None else n, mem, S.STAGE_ALL, C.byref(rh))
        if rc == 0:
            L.str_er_result_free(rh)
        return rc, (L.str_er_last_error(f.h) or b"").decode()

    p = fr.ctypes.data
    ok = R(p, 320, 240, 960)
    cases = [([ok, ok, ok], None, 0, -7, "3 frames"),                     # n > max_frames: STR_ER_ECAPACITY
             ([ok, R(p, 321, 200, 963)], None, 0, -7, "frame 1"),         # wider than the capacity
             ([R(p, 100, 241, 300)], None, 0, -7, "frame 0"),             # taller
             ([ok, R(p, 100, 100, 299)], None, 0, -1, "frame 1"),         # stride < 3 w: STR_ER_EINVAL
             ([ok, R(None, 10, 10, 30)], None, 0, -1, "frame 1"),         # NULL data
             ([ok], 0, 0, -1, "empty"),                                    # n = 0
             ([ok], None, 7, -1, "mem_kind")]                              # bad mem_kind
    for refs, n, mem, code, msg in cases:
        rc, err = call(refs, n, mem)
        assert rc == code and msg in err, (rc, err)
        again = f.text_detect_list([fr])
        assert again.cands.tobytes() == good.cands.tobytes()
    arr = (R * 1)(R(p, 50, 50, 49))
    rh = C.c_void_p()
    assert L.str_er_detect_planes_list(f.h, arr, 1, 0, S.STAGE_ALL, C.byref(rh)) == -1 and b"plane 0" in L.str_er_last_error(f.h)
    f.close()


def test_host_mirror_batch_matches_per_frame(S, cascade_paths, tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(S.lib_path())
    exe = str(tmp_path / "example_image_batch")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(root, "scene-text-recognition_amd", "host", "example_image_batch.cpp"),
                    "-I", os.path.join(root, "include"), "-L", libdir, "-lstr_er_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    sy = S.synth
    args = [exe, cascade_paths[0], cascade_paths[1]]
    for k, fr in enumerate([sy.stext_bgr(sy.frame_seed(80), 640, 480), _crops()[3], sy.stext_bgr(sy.frame_seed(81), 211, 97)]):
        raw = tmp_path / f"f{k}.bgr"
        raw.write_bytes(np.ascontiguousarray(fr).tobytes())
        args += [str(raw), str(fr.shape[1]), str(fr.shape[0])]
    out = subprocess.run(args, check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[-1] == "batch == per frame: yes"
    assert sum(1 for l in out if l.startswith("frame 2 plane")) == 6
