"""GPU test of the order of the argument checks of the ten query entry points (rt_terrain_trace_rays,
rt_terrain_trace_surface, rt_terrain_shade_rays, rt_terrain_sample_field, rt_terrain_sample_lattice and their device
forms; include/frosttrace.h).  Each call carries two faults at once and the test asserts which one is reported: the
order is part of the behaviour (null compute, count, options, no current shader, the family's own clause, missing
arrays, the texture, the device's flag, n == 0, and only then the device).  Every bad call is refused on the host
before any HIP call; no launch here is larger than 8 elements."""
import ctypes as C

import numpy as np
import pytest

import golden_index as GI
import ray_fixture as RF
import shade_ref as SH
from test_gpu_parity import make

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED, RT_ERR_STATE = 0, -1, -4, -5
N = 8
LATTICE = (4, 2, 1)  # 8 points


def _make(land="nomadplains"):
    """A 64x48 device and its terrain: the golden reset pose under the shaded tests' sun."""
    consts = dict(GI.consts(64, 48, "reset"))
    consts["sun"] = SH.SUN
    return make(consts, land, float_output=False)


class _Entries:
    """The ten entry points over one set of 8-element arrays.  call(name, cs, n, opt, null): null False: every array
    set; True: every array null; "outputs": the inputs set, the outputs null.  The lattice forms take dims for n."""

    def __init__(self):
        import torch
        import gpgpuraytrace_amd as G
        self.G, self.L = G, G.lib()
        o, d = RF.query(("G",))
        self.o, self.d = np.ascontiguousarray(o[:N]), np.ascontiguousarray(d[:N])
        self.pts = np.ascontiguousarray(self.o + np.float32(1.0))
        self.res = np.zeros((N, 8), np.float32)
        self.px, self.steps, self.occ = np.zeros(N, np.uint32), np.zeros((N, 2), np.uint32), np.zeros(N, np.uint32)
        self.drays = torch.from_numpy(G.pack_rays(self.o, self.d)).to("cuda:0")
        self.dpts = torch.from_numpy(G.pack_points(self.pts)).to("cuda:0")
        self.dres = torch.zeros((N, 8), dtype=torch.float32, device="cuda:0")
        self.dpx = torch.zeros(N, dtype=torch.int32, device="cuda:0")
        self.dsteps = torch.zeros((N, 2), dtype=torch.int32, device="cuda:0")
        self.docc = torch.zeros(N, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        self.names = ("trace_rays", "trace_rays_device", "trace_surface", "trace_surface_device", "shade_rays",
                      "shade_rays_device", "sample_field", "sample_field_device", "sample_lattice",
                      "sample_lattice_device")

    @staticmethod
    def family(name):
        return name.replace("_device", "")

    def options(self, name, size=None, mode=None):
        """The family's option block; size: its size field; mode: "segments" forced (rays, surface, shaded)."""
        fam, E = self.family(name), self.G.engine
        if fam == "trace_rays":
            opt = E.ray_options(None, mode or "auto", 0)
        elif fam in ("trace_surface", "shade_rays"):
            opt = E.surface_options(None, mode or "auto", 0)
        else:
            opt = E.field_options()
        if size is not None:
            opt.size = size
        return opt

    def call(self, name, cs, n=N, opt=None, null=False):
        fam, device, L = self.family(name), name.endswith("_device"), self.L
        ins, outs = null is not True, null is False
        ref = C.byref(opt) if opt is not None else None

        def h(a, on):
            return a.ctypes.data if on else None

        def g(t, on):
            return t.data_ptr() if on else None

        if fam in ("trace_rays", "trace_surface"):
            if device:
                return getattr(L, "rt_terrain_" + name)(cs, g(self.drays, ins), n, ref, g(self.dres, outs),
                                                        g(self.dsteps, outs))
            if fam == "trace_rays":
                return L.rt_terrain_trace_rays(cs, h(self.o, ins), h(self.d, ins), n, ref, h(self.res, outs),
                                               h(self.steps, outs))
            return L.rt_terrain_trace_surface(cs, h(self.o, ins), h(self.d, ins), None, n, ref, h(self.res, outs),
                                              h(self.steps, outs))
        if fam == "shade_rays":
            if device:
                return L.rt_terrain_shade_rays_device(cs, g(self.drays, ins), n, ref, g(self.dres, outs),
                                                      g(self.dpx, outs), g(self.dsteps, outs))
            return L.rt_terrain_shade_rays(cs, h(self.o, ins), h(self.d, ins), None, n, ref, h(self.res, outs),
                                           h(self.px, outs), h(self.steps, outs))
        if fam == "sample_field":
            if device:
                return L.rt_terrain_sample_field_device(cs, g(self.dpts, ins), n, ref, g(self.dres, outs))
            return L.rt_terrain_sample_field(cs, h(self.pts, ins), n, ref, h(self.res, outs))
        lat = self.G.engine.lattice((0, 30, 0), (1, 1, 1), n if isinstance(n, tuple) else LATTICE)
        if device:
            return L.rt_terrain_sample_lattice_device(cs, C.byref(lat), ref, g(self.dres, outs), g(self.docc, outs))
        return L.rt_terrain_sample_lattice(cs, C.byref(lat), ref, h(self.res, outs), h(self.occ, outs))


def test_which_of_two_faults_is_reported():
    e = _Entries()
    L = e.L
    dev, ter = _make()

    def compute(name, t=None):
        """The compute a family's queries take: the shaded queries tracescreen's, the others camerarays'."""
        t = t or ter
        return (t.compute if e.family(name) == "shade_rays" else t.camera_compute)._h

    def err():
        return L.rt_last_error()

    bare_cam, bare_scr = dev.create_compute(), dev.create_compute()  # computes with no texture bound
    assert bare_cam.create("shaders", "camerarays.hlsl", "CSMain", (16, 16, 1)) and bare_cam.swap()
    assert bare_scr.create("shaders", "tracescreen.hlsl", "CSMain", (16, 16, 1)) and bare_scr.swap()

    def bare(name):
        return (bare_scr if e.family(name) == "shade_rays" else bare_cam)._h

    for name in e.names:
        lattice = e.family(name) == "sample_lattice"
        cs = compute(name)
        # one query of 8 first: the lazy allocations have happened
        assert e.call(name, cs) == RT_OK, (name, err())
        dev.synchronize()
        # a null compute before the count (the lattice forms take no count: before the lattice)
        assert e.call(name, None, n=(4097, 1, 1) if lattice else -1) == RT_ERR_INVALID, name
        assert b"null compute" in err(), name
        # the count before the options
        if not lattice:
            assert e.call(name, cs, n=-1, opt=e.options(name, size=8)) == RT_ERR_INVALID and b"2^26" in err(), name
        # the options before the arrays
        assert e.call(name, cs, opt=e.options(name, size=8), null=True) == RT_ERR_INVALID and b"size" in err(), name
        # the family's clause before the arrays
        if e.family(name) == "shade_rays":
            assert e.call(name, ter.camera_compute._h, null=True) == RT_ERR_INVALID and b"camerarays" in err(), name
        if lattice:
            assert e.call(name, cs, n=(4097, 1, 1), null=True) == RT_ERR_INVALID and b"4096" in err(), name
        # the arrays before the texture
        both = lattice or e.family(name) == "shade_rays"
        assert e.call(name, bare(name), null="outputs" if both else True) == RT_ERR_INVALID, name
        assert (b"both null" if both else b"null") in err(), (name, err())
        # the texture before n == 0
        assert e.call(name, bare(name), n=(0, 2, 2) if lattice else 0) == RT_ERR_STATE and b"texPerm2D" in err(), name
        # n == 0 with every array null: RT_OK, nothing required (rt_device_kernel_time counts tracescreen launches
        # only, so there is no launch count to hold against the call)
        assert e.call(name, cs, n=(0, 2, 2) if lattice else 0, null=True) == RT_OK, (name, err())
    dev.check()
    dev.destroy()

    # the ray and surface queries' clause, segments on another landscape than nomadplains, before the arrays
    dev, ter = _make("testing")
    for name in e.names[:4]:
        opt = e.options(name, mode="segments")
        assert e.call(name, compute(name, ter), opt=opt, null=True) == RT_ERR_UNSUPPORTED, name
        assert b"segment" in err(), name
    dev.check()
    dev.destroy()
