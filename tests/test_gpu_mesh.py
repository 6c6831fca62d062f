"""GPU tests of the mesh extraction (rt_terrain_extract_mesh and its device form, ABI 9 additive): a surface-nets
mesh of a lattice's density, extracted on the device.  Bar: the vertex count, the triangle count, every position
word, cell word, normal / density word and index equal the checker's (tests/mesh_ref.py over the oracle's densities)
bit for bit, at every shape, grid and capacity, and an extraction between two renders changes nothing about the
frame loop."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as MR
import ray_fixture as RF
from test_gpu_field_query import DEFER, EYE, NEAR, NOMAD, SMALL_SPACING, SMALL_Y, _bits, _make, _pose, _golden_pair
from test_gpu_parity import make

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_STATE = 0, -1, -5
POISON = 0xdeadbeef
# (2,2,2): one cell, no quads; (3,3,3): the smallest lattice with an interior edge; (66,4,3): 65 cells a row, the
# lane 63 / 64 neighbour; (130,6,5): three mask words a row; (97,1,4): no cells
SMALL = ((2, 2, 2), (3, 3, 3), (33, 5, 3), (66, 4, 3), (130, 6, 5), (97, 1, 4))
FULL = ((33, 5, 3), (66, 4, 3), (130, 6, 5))  # the non-degenerate ones: the surface runs through them
# The one non-degenerate case whose quads all have the same winding: in greenrocks' (33,5,3) lattice the oracle's
# field has the lower endpoint of all 25 crossing interior edges inside.  Pinned as a fact about the field (the test
# asserts it), so that every other case is held to both windings.
ONE_WINDING = {("greenrocks", (33, 5, 3))}


def _small(land, dims):
    origin = (0.7, SMALL_Y[land], 0.7)
    return origin, SMALL_SPACING, dims, MR.lattice_mesh("small%dx%dx%d" % dims, origin, SMALL_SPACING, dims, EYE, land)


def _full(m, what=""):
    """Conditions on the checker, not on the device: vertices, quads on all three axes, both windings."""
    assert len(m.vertices) > 0 and set(m.quad_axis.tolist()) == {0, 1, 2}, what
    if what in ONE_WINDING:
        assert m.quad_inside.all() and len(m.quad_inside) == 25, what
    else:
        assert m.quad_inside.any() and not m.quad_inside.all(), what


def _check(got, m, nrm, what=""):
    import gpgpuraytrace_amd as G
    assert got is not None, (what, G.lib().rt_last_error())
    v, n, t, cells = got
    assert (len(v), len(t)) == (len(m.vertices), len(m.triangles)), what
    _bits(v, m.vertices, what)
    assert cells.dtype == np.uint32 and np.array_equal(cells, m.cells), what
    assert t.dtype == np.uint32 and t.shape == m.triangles.shape and np.array_equal(t, m.triangles), what
    if nrm is None:
        assert n is None, what
    else:
        _bits(n, nrm, what)


@pytest.mark.parametrize("land", RF.LANDSCAPES)
def test_small_lattices(land):
    dev, ter = _make(land)
    for dims in SMALL:
        origin, spacing, _, m = _small(land, dims)
        key = "small%dx%dx%d" % dims
        if dims in FULL:
            _full(m, (land, dims))
        elif dims == (2, 2, 2):
            assert len(m.vertices) <= 1 and len(m.triangles) == 0
        elif dims == (3, 3, 3):
            assert len(m.triangles) <= 6
        else:
            assert len(m.vertices) == 0 and len(m.triangles) == 0
        nrm = MR.normals(key, m.vertices, EYE, land)
        assert np.isfinite(nrm).all()
        _check(ter.extract_mesh(origin, spacing, dims, eye=EYE), m, nrm, (land, dims))
    dev.check()
    dev.destroy()


def test_the_near_lattice_on_grids_of_one_and_two_blocks():
    origin, spacing, dims, eye = NEAR
    m = MR.lattice_mesh("near", origin, spacing, dims, eye, "nomadplains")
    _full(m)
    assert len(m.vertices) > 2048  # the normal pass takes more than two tiles
    nrm = MR.normals("near", m.vertices, eye, "nomadplains")
    dev, ter = _make()
    for mb in (0, 1, 2):
        _check(ter.extract_mesh(origin, spacing, dims, eye=eye, max_blocks=mb), m, nrm, mb)
    dev.check()
    dev.destroy()


def test_a_lattice_of_three_scan_chunks():
    """3 x 95 x 95 points: 94 x 94 = 8836 one-word cell rows, so the scan walks three chunks of 4096 words and
    carries its totals across them, and the count and emit grids of one block stride many times."""
    origin, spacing, dims = (-3.0, 0.0, -100.0), (2.5, 0.7, 2.2), (3, 95, 95)
    m = MR.lattice_mesh("rows", origin, spacing, dims, EYE, "nomadplains")
    _full(m)
    words = m.cells.astype(np.int64) // 2  # two cells a row, one mask word a row: the word is the cell row
    assert (dims[1] - 1) * (dims[2] - 1) > 8192
    assert (words < 4096).any() and ((words >= 4096) & (words < 8192)).any() and (words >= 8192).any()
    nrm = MR.normals("rows", m.vertices, EYE, "nomadplains")
    dev, ter = _make()
    for mb in (0, 1):
        _check(ter.extract_mesh(origin, spacing, dims, eye=EYE, max_blocks=mb), m, nrm, mb)
    dev.check()
    dev.destroy()


def test_a_negative_spacing():
    origin, spacing, dims, eye = NOMAD["negative"]
    m = MR.lattice_mesh("negative", origin, spacing, dims, eye, "nomadplains")
    _full(m)
    dev, ter = _make()
    _check(ter.extract_mesh(origin, spacing, dims, eye=eye), m, MR.normals("negative", m.vertices, eye, "nomadplains"))
    dev.check()
    dev.destroy()


def _raw(ter, origin, spacing, dims, eye, cap_v, cap_t, normals=True, size_v=None, size_t=None):
    """The host form with poisoned arrays of size_v / size_t entries and capacities cap_v / cap_t."""
    import gpgpuraytrace_amd as G
    size_v, size_t = cap_v if size_v is None else size_v, cap_t if size_t is None else size_t
    v = np.full((size_v, 4), POISON, np.uint32)
    n = np.full((size_v, 4), POISON, np.uint32)
    t = np.full((size_t, 3), POISON, np.uint32)
    counts = np.full(2, POISON, np.uint32)
    lat, opt = G.engine.lattice(origin, spacing, dims), G.engine.field_options(eye)
    rc = G.lib().rt_terrain_extract_mesh(ter.camera_compute._h, C.byref(lat), C.byref(opt),
                                         v.ctypes.data if size_v else None, n.ctypes.data if normals and size_v else None,
                                         cap_v, t.ctypes.data if size_t else None, cap_t, counts.ctypes.data)
    return rc, v, n, t, counts


def _words(m, nrm):
    """The checker's arrays as the C-ABI lays them out: vertices x y z cell, normals, triangles, all uint32."""
    v = np.concatenate([m.vertices.view(np.uint32), m.cells[:, None]], axis=1)
    return v, np.ascontiguousarray(nrm).view(np.uint32), m.triangles


def test_truncated_calls_write_exactly_the_prefix():
    land, dims = "nomadplains", (66, 4, 3)
    origin, spacing, _, m = _small(land, dims)
    _full(m)
    want_v, want_n, want_t = _words(m, MR.normals("small66x4x3", m.vertices, EYE, land))
    nv, nt = len(want_v), len(want_t)
    assert nv >= 8 and nt >= 8
    dev, ter = _make(land)
    for cap_v, cap_t in ((nv // 2, nt // 2), (nv, nt), (0, nt // 2), (nv // 2, 0), (1, 1), (nv + 5, nt + 5)):
        rc, v, n, t, counts = _raw(ter, origin, spacing, dims, EYE, cap_v, cap_t, size_v=nv + 9, size_t=nt + 9)
        assert rc == RT_OK and counts.tolist() == [nv, nt], (cap_v, cap_t)  # the FULL counts, whatever the capacity
        kv, kt = min(cap_v, nv), min(cap_t, nt)
        assert np.array_equal(v[:kv], want_v[:kv]) and (v[kv:] == POISON).all(), (cap_v, cap_t)
        assert np.array_equal(n[:kv], want_n[:kv]) and (n[kv:] == POISON).all(), (cap_v, cap_t)
        assert np.array_equal(t[:kt], want_t[:kt]) and (t[kt:] == POISON).all(), (cap_v, cap_t)
    # an odd triangle capacity splits a quad: its first triangle is written, its second is not
    rc, v, n, t, counts = _raw(ter, origin, spacing, dims, EYE, 0, 3, size_t=nt)
    assert rc == RT_OK and np.array_equal(t[:3], want_t[:3]) and (t[3:] == POISON).all()
    # a counting call: capacities 0, arrays NULL
    rc, _, _, _, counts = _raw(ter, origin, spacing, dims, EYE, 0, 0)
    assert rc == RT_OK and counts.tolist() == [nv, nt]
    dev.check()
    dev.destroy()


def test_without_normals_no_normal_pass_runs():
    land, dims = "nomadplains", (33, 5, 3)
    origin, spacing, _, m = _small(land, dims)
    dev, ter = _make(land)
    _check(ter.extract_mesh(origin, spacing, dims, eye=EYE, normals=False), m, None)
    nv, nt = len(m.vertices), len(m.triangles)
    rc, v, n, t, counts = _raw(ter, origin, spacing, dims, EYE, nv, nt, normals=False)
    assert rc == RT_OK and counts.tolist() == [nv, nt]
    want_v, _, want_t = _words(m, np.zeros((nv, 4), np.float32))
    assert np.array_equal(v, want_v) and np.array_equal(t, want_t)
    assert (n == POISON).all()  # (never handed over)
    dev.check()
    dev.destroy()


def test_device_form_equals_the_host_form():
    """torch-allocated scratch, arrays and counts, poisoned, with room to spare: the device form writes what the host
    form returns and nothing beyond it; without a normals array the poisoned one stays; too little scratch is an
    error."""
    import torch
    import gpgpuraytrace_amd as G
    origin, spacing, dims, eye = NEAR
    m = MR.lattice_mesh("near", origin, spacing, dims, eye, "nomadplains")
    nv, nt = len(m.vertices), len(m.triangles)
    dev, ter = _make()
    host = ter.extract_mesh(origin, spacing, dims, eye=eye)
    _check(host, m, MR.normals("near", m.vertices, eye, "nomadplains"))
    need = G.engine.mesh_scratch_bytes(origin, spacing, dims)
    assert need > 0
    cap_v, cap_t = nv + 17, nt + 17

    def poisoned(*shape):
        return torch.full(shape, -559038737, dtype=torch.int32, device="cuda:0")  # 0xdeadbeef

    scratch = torch.zeros(need, dtype=torch.uint8, device="cuda:0")
    v, n, n2, t, counts = poisoned(cap_v, 4), poisoned(cap_v, 4), poisoned(cap_v, 4), poisoned(cap_t, 3), poisoned(2)
    torch.cuda.synchronize()
    args = (origin, spacing, dims, scratch.data_ptr(), need, v.data_ptr())
    assert ter.extract_mesh_device(*args, n.data_ptr(), cap_v, t.data_ptr(), cap_t, counts.data_ptr(), eye=eye)
    dev.synchronize()
    got = [x.cpu().numpy().view(np.uint32) for x in (v, n, t, counts)]
    assert got[3].tolist() == [nv, nt]
    want_v, want_n, want_t = _words(m, host[1])
    for g, w, k in ((got[0], want_v, nv), (got[1], want_n, nv), (got[2], want_t, nt)):
        assert np.array_equal(g[:k], w) and (g[k:] == POISON).all()
    # no normals array: the other arrays are written again, a poisoned array is not touched
    v.fill_(-559038737)
    torch.cuda.synchronize()
    assert ter.extract_mesh_device(*args, 0, cap_v, t.data_ptr(), cap_t, counts.data_ptr(), eye=eye)
    dev.synchronize()
    assert np.array_equal(v.cpu().numpy().view(np.uint32)[:nv], want_v)
    assert (n2.cpu().numpy().view(np.uint32) == POISON).all()
    # a counting call on the device, and one without cells: the counts alone
    counts.fill_(-559038737)
    torch.cuda.synchronize()
    assert ter.extract_mesh_device(origin, spacing, dims, scratch.data_ptr(), need, 0, 0, 0, 0, 0, counts.data_ptr(), eye=eye)
    dev.synchronize()
    assert counts.cpu().numpy().view(np.uint32).tolist() == [nv, nt]
    assert ter.extract_mesh_device(origin, spacing, (97, 1, 4), 0, 0, 0, 0, 0, 0, 0, counts.data_ptr(), eye=eye)
    dev.synchronize()
    assert counts.cpu().numpy().tolist() == [0, 0]
    # too little scratch, none, or a misaligned block
    assert not ter.extract_mesh_device(origin, spacing, dims, scratch.data_ptr(), need - 1, v.data_ptr(), 0, cap_v,
                                       t.data_ptr(), cap_t, counts.data_ptr(), eye=eye)
    assert b"scratch" in G.lib().rt_last_error()
    assert not ter.extract_mesh_device(origin, spacing, dims, 0, need, v.data_ptr(), 0, cap_v, t.data_ptr(), cap_t,
                                       counts.data_ptr(), eye=eye)
    assert not ter.extract_mesh_device(origin, spacing, dims, scratch.data_ptr() + 4, need - 4, v.data_ptr(), 0, cap_v,
                                       t.data_ptr(), cap_t, counts.data_ptr(), eye=eye)
    dev.check()
    dev.destroy()


def test_arguments():
    import gpgpuraytrace_amd as G
    from gpgpuraytrace_amd import _native
    L = G.lib()
    dev, ter = _make()
    cs = ter.camera_compute._h
    origin, spacing, dims = (0.7, SMALL_Y["nomadplains"], 0.7), SMALL_SPACING, (33, 5, 3)
    m = MR.lattice_mesh("small33x5x3", origin, spacing, dims, EYE, "nomadplains")
    nv, nt = len(m.vertices), len(m.triangles)
    good = G.engine.lattice(origin, spacing, dims)
    v, t = np.zeros((nv, 4), np.float32), np.zeros((nt, 3), np.uint32)
    counts = np.zeros(2, np.uint32)
    vp, tp, cp = v.ctypes.data, t.ctypes.data, counts.ctypes.data

    def ref(o):
        return C.byref(o) if o is not None else None

    def call(lat=good, opt=G.engine.field_options(EYE), v_=vp, cap_v=nv, t_=tp, cap_t=nt, c_=cp):
        return L.rt_terrain_extract_mesh(cs, ref(lat), ref(opt), v_, None, cap_v, t_, cap_t, c_)

    assert call() == RT_OK and counts.tolist() == [nv, nt]
    assert call(opt=None) == RT_OK  # the compute's Eye
    assert call(lat=None) == RT_ERR_INVALID
    assert call(c_=None) == RT_ERR_INVALID and b"counts" in L.rt_last_error()
    assert call(v_=None) == RT_ERR_INVALID and b"capacity" in L.rt_last_error()
    assert call(t_=None) == RT_ERR_INVALID
    assert call(v_=None, cap_v=0, t_=None, cap_t=0) == RT_OK
    for size in (0, 8, 23):
        short = G.engine.field_options()
        short.size = size
        assert call(opt=short) == RT_ERR_INVALID and b"size" in L.rt_last_error()
    for flags in (2, 4, 8, 16, 64, 1 << 31):
        bad = G.engine.field_options()
        bad.flags = flags
        assert call(opt=bad) == RT_ERR_INVALID and b"flags" in L.rt_last_error(), flags
    # RT_FIELD_NORMAL is ignored: the same vertices
    assert call() == RT_OK
    first = v.copy()
    assert call(opt=G.engine.field_options(EYE, True)) == RT_OK and np.array_equal(v.view(np.uint32), first.view(np.uint32))
    _bits(np.ascontiguousarray(v[:, :3]), m.vertices)
    for bad_dims in ((4097, 2, 2), (4096, 4096, 5)):
        assert call(lat=G.engine.lattice((0, 0, 0), (1, 1, 1), bad_dims)) == RT_ERR_INVALID
    assert call(lat=G.engine.lattice((float("nan"), 0, 0), (1, 1, 1), (4, 4, 4))) == RT_ERR_INVALID
    # a capacity far above the mesh is no more than the cells: the arrays hold the counts' entries
    assert call(cap_v=nv, cap_t=nt) == RT_OK
    # no cells: counts 0, nothing else needed
    counts[:] = 7
    assert call(lat=G.engine.lattice(origin, spacing, (97, 1, 4)), v_=None, cap_v=0, t_=None, cap_t=0) == RT_OK
    assert counts.tolist() == [0, 0]
    got = ter.extract_mesh(origin, spacing, (97, 1, 4), eye=EYE)
    assert got is not None and got[0].shape == (0, 3) and got[1].shape == (0, 4) and got[2].shape == (0, 3)
    # either kind of compute
    assert L.rt_terrain_extract_mesh(ter.compute._h, ref(good), ref(G.engine.field_options(EYE)), vp, None, nv, tp, nt,
                                     cp) == RT_OK
    assert np.array_equal(v.view(np.uint32), first.view(np.uint32))
    # the Python mirror: None, no exception
    assert ter.extract_mesh((0, 0, 0), (1, 1, 1), (4097, 2, 2)) is None
    # no texture bound: RT_ERR_STATE, as the other queries
    bare = dev.create_compute()
    assert bare.create("shaders", "camerarays.hlsl", "CSMain", (16, 16, 1)) and bare.swap()
    assert L.rt_terrain_extract_mesh(bare._h, ref(good), None, vp, None, nv, tp, nt, cp) == RT_ERR_STATE
    assert b"texPerm2D" in L.rt_last_error()
    assert _native.SIGNATURES["rt_terrain_extract_mesh"][0] is C.c_int
    dev.check()
    dev.destroy()


@pytest.mark.parametrize("batch", [1, 2])
def test_deferred_loop_is_undisturbed(batch):
    """A deferred device at one and at two frames to a launch: an extraction between two renders launches no
    pending frame (the same deferred_fused and launch_info as without), and the frames are golden."""
    land, cams, frames = _golden_pair()
    n = 6
    origin, spacing, dims = (0.7, SMALL_Y["nomadplains"], 0.7), SMALL_SPACING, (33, 5, 3)
    m = MR.lattice_mesh("small33x5x3", origin, spacing, dims, EYE, "nomadplains")
    nrm = MR.normals("small33x5x3", m.vertices, EYE, "nomadplains")

    def loop(queries):
        dev, ter = make(cams[0], land, float_output=False, **DEFER)
        dev.defer_batch(batch)
        infos = []
        for k in range(n):
            _pose(ter, cams[k % 2])
            ter.render_device()
            before = (dev.deferred_fused(), dev.launch_info())
            if queries:
                _check(ter.extract_mesh(origin, spacing, dims, eye=EYE, normals=bool(k % 2)), m, nrm if k % 2 else None, k)
                assert (dev.deferred_fused(), dev.launch_info()) == before, k
            infos.append(before)
        assert np.array_equal(dev.readback(), frames[(n - 1) % 2])  # (launches what is pending)
        infos.append((dev.deferred_fused(), dev.launch_info()))
        dev.check()
        dev.destroy()
        return infos

    with_q, without = loop(True), loop(False)
    assert with_q == without and with_q[-1][0] == n - batch
