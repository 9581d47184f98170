"""Lists of frames of different sizes on the ingest stream (str_er_stream_submit_list / _nv12_list / _copy_list) and NV12 lists
(str_er_detect_nv12_list): every record against the list call, ticket order with uniform submissions in between, NV12 planes against the
oracle and every NV12 frame against str_er_detect_nv12 alone, device frames, the submit-time errors, and the image-stream example."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import check_plane_against_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ALL_STAGES_FIELDS = ("info", "cands", "ocr_label", "ocr_prob", "tracks", "texts", "text_ers", "group_all", "group_bounds", "line_label",
                     "line_prob", "line_kept", "text_alive")


def _crops():
    z = np.load(os.path.join(GOLDEN, "icdar_crops.npz"))
    return [np.ascontiguousarray(z[k]) for k in sorted(z.files)]


def _same(a, b, fields=ALL_STAGES_FIELDS):
    for k in fields:
        x, y = getattr(a, k, None), getattr(b, k, None)
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.tobytes() == y.tobytes(), k


def _place(buf, frames, at0, bpp=3, rows_of=None):
    """Write frames into buf one after the other, frame k from an odd offset with an odd row stride: [(offset, w, h, stride)]."""
    layout, at = [], at0
    for k, fr in enumerate(frames):
        rows = fr.shape[0]
        w = fr.shape[1]
        row = bpp * w
        stride = row + 5 + 2 * k
        at += 1 + 2 * k                                     # (a gap of 1 + 2 k bytes: frames start at unaligned offsets)
        for y in range(rows):
            buf[at + y * stride:at + y * stride + row] = fr[y].reshape(-1)
        layout.append((at, w, rows_of(rows) if rows_of else rows, stride))
        at += (rows - 1) * stride + row
    return layout


def _stream_ctx(S, cascade_paths, prm, depth, svm=None):
    import ctypes as C
    st = S.FrameStream(prm, depth=depth)
    st.load_cascade(0, cascade_paths[0]); st.load_cascade(1, cascade_paths[1])
    if svm is not None:
        for i in range(depth):
            ctx = st.L.str_er_stream_context(st.h, i)
            assert st.L.str_er_load_svm_model_mem(ctx, svm, len(svm), 1800) == 0
    return st


@pytest.mark.parametrize("depth", [1, 3])
def test_stream_list_equals_the_list_call(S, cascade_paths, depth):
    prm = S.Params(max_width=640, max_height=480, max_frames=4)
    svm = gzip.open(S.cascade_io.ocr_model_path()).read()
    st = _stream_ctx(S, cascade_paths, prm, depth, svm)
    ref = S.ERFilter(params=prm)
    ref.load_cascade(0, cascade_paths[0]); ref.load_cascade(1, cascade_paths[1])
    ref.load_svm_model_text(svm, 1800)
    sy, cr = S.synth, _crops()
    lists = [[cr[0], sy.stext_bgr(sy.frame_seed(200), 640, 480), sy.stext_bgr(sy.frame_seed(201), 321, 243)],
             [cr[1], cr[2], sy.snoise_bgr(sy.frame_seed(202), 97, 61), cr[3]],
             [sy.stext_bgr(sy.frame_seed(203), 480, 200)],
             [cr[3], sy.stext_bgr(sy.frame_seed(204), 333, 477)]]
    stages = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP | S.STAGE_OCR | S.STAGE_OCR_LINES
    expected = [ref.text_detect_list(fr, stages) for fr in lists]
    assert sum(len(e.texts) for e in expected) > 0
    got, tickets = [], []
    for i, fr in enumerate(lists):
        if st.pending() == depth:
            t, r = st.next()
            tickets.append(t); got.append(r)
        slot, buf = st.acquire()
        st.submit_list(slot, _place(buf, fr, 3 * i), stages)
    while st.pending():
        t, r = st.next()
        tickets.append(t); got.append(r)
    assert tickets == list(range(1, len(lists) + 1))
    for g, e in zip(got, expected):
        _same(g, e)
    st.close(); ref.close()


def test_uniform_and_list_submissions_interleave(S, cascade_paths):
    W, H = 320, 240
    prm = S.Params(max_width=W, max_height=H, max_frames=3)
    st = _stream_ctx(S, cascade_paths, prm, 2)
    ref = S.ERFilter(params=prm)
    ref.load_cascade(0, cascade_paths[0]); ref.load_cascade(1, cascade_paths[1])
    sy, cr = S.synth, _crops()
    uni = np.stack([sy.stext_bgr(sy.frame_seed(300 + k), W, H) for k in range(2)])
    mixed = [cr[0], sy.stext_bgr(sy.frame_seed(310), 211, 97), cr[2]]
    one = sy.stext_bgr(sy.frame_seed(311), W, H)
    stages = S.STAGE_ALL | S.STAGE_TRACK | S.STAGE_GROUP
    jobs = [("uniform", uni), ("list", mixed), ("one", one), ("copy_list", mixed[::-1]), ("uniform", one[None]), ("list", [one, cr[0]])]
    want = {"uniform": lambda x: ref.text_detect(x, stages), "list": lambda x: ref.text_detect_list(x, stages),
            "one": lambda x: ref.text_detect(x, stages), "copy_list": lambda x: ref.text_detect_list(x, stages)}
    expected = [want[k](x) for k, x in jobs]
    got, tickets = [], []
    for i, (kind, x) in enumerate(jobs):
        if st.pending() == 2:
            t, r = st.next()
            tickets.append(t); got.append(r)
        if kind == "copy_list":
            st.submit_copy_list(x, stages)
            continue
        slot, buf = st.acquire()
        if kind == "uniform":
            buf[:x.size] = x.reshape(-1)
            st.submit(slot, W, H, len(x), stages)
        else:
            st.submit_list(slot, _place(buf, [x] if kind == "one" else x, 7 * i), stages)
    while st.pending():
        t, r = st.next()
        tickets.append(t); got.append(r)
    assert tickets == list(range(1, len(jobs) + 1))
    for g, e in zip(got, expected):
        _same(g, e, ("info", "cands", "tracks", "texts", "text_ers", "group_all", "group_bounds"))
    _same(got[2], got[4], ("info", "cands", "tracks", "texts", "text_ers"))     # a one-frame list == the uniform submission of that frame
    assert len(got[2].cands) > 0
    st.close(); ref.close()


def _frame_matches_alone(lst, one, i):
    """Frame i of a list result against the result of that frame alone (frame = 0): the same records, plane indices shifted."""
    poff = int(np.nonzero(lst.info["frame"] == i)[0][0])
    exp = one.info.copy()
    exp["frame"] = i
    assert lst.info[lst.info["frame"] == i].tobytes() == exp.tobytes()
    got = lst.cands[lst.cands["frame"] == i].copy()
    got["plane"] -= poff
    exp = one.cands.copy()
    exp["frame"] = i
    assert got.tobytes() == exp.tobytes()
    for k in range(len(one.info)):
        assert lst.planes[poff + k].nodes.tobytes() == one.planes[k].nodes.tobytes()


def test_nv12_list_matches_the_oracle_and_single_calls(S, cascade_paths, oracle, oracle_cascades):
    L = 2
    prm = S.Params(max_width=640, max_height=480, max_frames=4, n_pyr_levels=L)
    f = S.ERFilter(params=prm)
    f.load_cascade(0, cascade_paths[0]); f.load_cascade(1, cascade_paths[1])
    sy, cr = S.synth, _crops()
    bgr = [sy.stext_bgr(sy.frame_seed(400), 640, 480), cr[3], sy.stext_bgr(sy.frame_seed(401), 198, 90), cr[1]]
    nv = [sy.nv12_from_bgr(b) for b in bgr]
    big = np.zeros((90 + 45 + 3, 198 + 11), np.uint8)       # frame 2 as a view with a row stride (not copied)
    big[1:1 + 135, 5:5 + 198] = nv[2]
    frames = [nv[0], nv[1], big[1:1 + 135, 5:5 + 198], nv[3]]
    res = f.text_detect_nv12_list(frames, want_nodes=True)
    assert len(res.planes) == 4 * L * 6 and len(res.cands) > 0
    for i in (0, 2):                                          # every plane of two frames through the oracle
        w, h = bgr[i].shape[1], bgr[i].shape[0]
        three = oracle.nv12_to_ycrcb(nv[i], w, h)
        pyr = {c: oracle.pyramid(three[c], L) for c in range(3)}
        ps = [p for p in res.planes if p.frame == i]
        assert len(ps) == L * 6
        for p in ps:
            img = pyr[p.ch % 3][p.pyr]
            assert (p.width, p.height) == (img.shape[1], img.shape[0])
            check_plane_against_oracle(oracle, p, 255 - img if p.ch >= 3 else img, oracle_cascades)
    for i, n in enumerate(nv):                                # every frame against str_er_detect_nv12 on it alone
        one = f.text_detect_nv12(n, bgr[i].shape[1], bgr[i].shape[0], want_nodes=True)
        _frame_matches_alone(res, one, i)
    # the same frames through the stream (NV12 list in the staging buffer, odd offsets and strides)
    st = _stream_ctx(S, cascade_paths, prm, 2)
    slot, buf = st.acquire()
    st.submit_nv12_list(slot, _place(buf, nv, 1, bpp=1, rows_of=lambda r: r // 3 * 2), S.STAGE_ALL | S.WANT_NODES)
    _, sres = st.next()
    _same(sres, res, ("info", "cands"))
    for a, b in zip(sres.planes, res.planes):
        assert a.nodes.tobytes() == b.nodes.tobytes()
    st.close(); f.close()


_NV12_DEVICE_CHILD = r"""
import sys
import numpy as np
import torch                                    # (first: the HIP runtime PyTorch brings, as in smoke())
sys.path.insert(0, sys.argv[1])
import importlib
S = importlib.import_module("scene-text-recognition_amd")
f = S.ERFilter(params=S.Params(max_width=640, max_height=480, max_frames=3, n_pyr_levels=3, channel_mask=0x07))
f.load_cascade(0, sys.argv[2]); f.load_cascade(1, sys.argv[3])
sy = S.synth
crop = np.ascontiguousarray(np.load(sys.argv[4])["crop2"])
nv = [sy.nv12_from_bgr(b) for b in (sy.stext_bgr(sy.frame_seed(410), 640, 480), crop, sy.stext_bgr(sy.frame_seed(411), 322, 244))]
host = f.text_detect_nv12_list(nv, want_nodes=True)
bufs, refs = [], []
for k, n in enumerate(nv):
    rows, w = n.shape
    pitch = w + 7 + 2 * k                       # odd row pitches, and the frame starts 1 + k bytes into its buffer
    buf = np.zeros(1 + k + pitch * rows, np.uint8)
    for y in range(rows):
        buf[1 + k + y * pitch:1 + k + y * pitch + w] = n[y]
    t = torch.from_numpy(buf).cuda()
    bufs.append(t)
    refs.append((t.data_ptr() + 1 + k, w, rows // 3 * 2, pitch))
torch.cuda.synchronize()
dev = f.detect_nv12_list_device(refs, S.STAGE_ALL | S.WANT_NODES)
assert dev.info.tobytes() == host.info.tobytes() and dev.cands.tobytes() == host.cands.tobytes()
for a, b in zip(dev.planes, host.planes):
    assert a.nodes.tobytes() == b.nodes.tobytes()
assert len(host.cands) > 0
print("device nv12 list == host nv12 list:", len(host.cands), "candidates")
"""


def test_nv12_device_frames_at_odd_pitches(S, cascade_paths):
    """NV12 frames in device memory (torch tensors) at odd pitches and unaligned starts == the same frames from the host; in a child process
    that loads PyTorch's HIP runtime before the library, as test_ragged_batch.py does."""
    r = subprocess.run([sys.executable, "-c", _NV12_DEVICE_CHILD, ROOT, cascade_paths[0], cascade_paths[1], os.path.join(GOLDEN, "icdar_crops.npz")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "device nv12 list == host nv12 list" in r.stdout


def test_submit_errors_name_the_frame_and_keep_the_slot(S, cascade_paths):
    W, H = 320, 240
    prm = S.Params(max_width=W, max_height=H, max_frames=2)
    st = _stream_ctx(S, cascade_paths, prm, 2)
    ref = S.ERFilter(params=prm)
    ref.load_cascade(0, cascade_paths[0]); ref.load_cascade(1, cascade_paths[1])
    sy = S.synth
    frames = [sy.stext_bgr(sy.frame_seed(500), 211, 97), sy.stext_bgr(sy.frame_seed(501), W, H)]
    good = ref.text_detect_list(frames)
    nv = sy.nv12_from_bgr(frames[1])
    good_nv = ref.text_detect_nv12_list([nv])
    slot, buf = st.acquire()
    cap = len(buf)
    ok = _place(buf, frames, 0)
    cases = [("bgr", [ok[0], (cap - 100, 50, 10, 150)], -1, "frame 1"),            # rows beyond the end of the buffer
             ("bgr", [ok[0], (-64, 10, 10, 30)], -1, "frame 1"),                  # before its start
             ("bgr", [(0, W + 1, 10, 3 * W + 3)], -7, "frame 0"),                 # wider than the capacity
             ("bgr", [(0, 10, H + 1, 30)], -7, "frame 0"),                        # taller
             ("bgr", [ok[0], ok[1], ok[0]], -7, "3 frames"),                      # more frames than max_frames
             ("bgr", [ok[0], (0, 100, 10, 299)], -1, "frame 1"),                  # stride below a row
             ("nv12", [(0, 100, 10, 100), (0, 101, 10, 101)], -1, "frame 1"),     # odd NV12 width
             ("nv12", [(0, 100, 11, 100)], -1, "frame 0")]                        # odd NV12 height
    for kind, layout, code, msg in cases:
        with pytest.raises(S.StrErError) as e:
            (st.submit_nv12_list if kind == "nv12" else st.submit_list)(slot, layout, S.STAGE_ALL)
        assert e.value.code == code and msg in str(e.value), (layout, str(e.value))
    # the slot is still acquired: the next submission on it is served correctly, and so is an NV12 one after it
    st.submit_list(slot, ok, S.STAGE_ALL)
    _same(st.next()[1], good, ("info", "cands"))
    slot, buf = st.acquire()
    buf[:nv.size] = nv.reshape(-1)
    st.submit_nv12_list(slot, [(0, W, H, W)], S.STAGE_ALL)
    _same(st.next()[1], good_nv, ("info", "cands"))
    # the list call on a context: odd NV12 dims, frame named, the context serves the next call
    with pytest.raises(S.StrErError) as e:
        ref.text_detect_nv12_list([nv, np.zeros((15, 9), np.uint8)])
    assert e.value.code == -1 and "frame 1" in str(e.value)
    _same(ref.text_detect_nv12_list([nv]), good_nv, ("info", "cands"))
    # submit_copy_list: a frame over the capacity leaves no slot acquired
    with pytest.raises(S.StrErError) as e:
        st.submit_copy_list([frames[0], np.zeros((H, W + 4, 3), np.uint8)])
    assert e.value.code == -7 and "frame 1" in str(e.value)
    st.submit_copy_list(frames)
    st.submit_copy_list(frames[::-1])
    _same(st.next()[1], good, ("info", "cands"))
    _same(st.next()[1], ref.text_detect_list(frames[::-1]), ("info", "cands"))
    st.close(); ref.close()


def test_example_image_stream_runs(S, cascade_paths, tmp_path):
    libdir = os.path.dirname(S.lib_path())
    exe = str(tmp_path / "example_image_stream")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "scene-text-recognition_amd", "host", "example_image_stream.cpp"),
                    "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lstr_er_hip", f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    r = subprocess.run([exe, cascade_paths[0], cascade_paths[1], "11", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert out[-1] == "stream == batch: yes"
    assert sum(1 for l in out if l.startswith("photo ")) == 11
    assert any(int(l.split(" pool ")[1].split()[0]) > 0 for l in out if l.startswith("photo "))
