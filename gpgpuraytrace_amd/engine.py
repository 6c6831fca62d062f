"""Host-side mirror of the reference engine's dispatch-and-readback surface over
the C-ABI (include/frosttrace.h).

Class/method names follow the reference interfaces so an engine-side caller
reads the same:  DeviceFactory.construct -> Device (IDevice, Factories/IDevice.h),
Device.create_compute -> Compute (ICompute, Factories/ICompute.h), ShaderVariable /
ShaderArray (Graphics/IShaderVariable.h), Texture (Factories/ITexture.h), Noise
(Graphics/Noise.cpp), Terrain (Graphics/Terrain.cpp).  Errors follow the
reference: bool returns / None for missing names; HIP failures raise.
"""
import ctypes as C
import os
import warnings

import numpy as np

from . import _native
from ._native import check, lib

CAMERA_VIEW_RES = 32    # Gameplay/Flyby.h:6
CAMERA_THREAD_RES = 16  # Gameplay/Flyby.h:7


class DeviceAPI:
    NONE, DIRECT3D, OPENGL, HIP = 0, 1, 2, 3   # IDevice.h:5-10 + the HIP slot


def vfs_add_path(path):
    """VFS::addPath (Common/VFS.cpp); "Media/<landscape>" selects the landscape."""
    check(lib().rt_vfs_add_path(path.encode()), "vfs_add_path")


def vfs_clear():
    lib().rt_vfs_clear()


class ShaderVariable:
    """IShaderVariable: write() copies exactly the reflected size into the cbuffer shadow."""

    def __init__(self, handle, compute):
        self._h, self._compute = handle, compute
        self.name = lib().rt_variable_name(handle).decode()
        self.size = int(lib().rt_variable_size(handle))

    def write(self, data):
        buf = bytes(np.ascontiguousarray(data).tobytes() if not isinstance(data, (bytes, bytearray)) else data)
        if len(buf) < self.size:
            raise ValueError(f"{self.name}: need {self.size} bytes, got {len(buf)}")
        check(lib().rt_variable_write(self._h, buf), f"write {self.name}")


class ShaderArray:
    """IShaderArray: create(n), map()/unmap() on UAV arrays, write() on SRV arrays."""

    def __init__(self, handle, compute):
        self._h, self._compute = handle, compute
        self.stride = int(lib().rt_array_stride(handle))
        self.elements = 0

    def create(self, elements):
        rc = lib().rt_array_create(self._h, int(elements))
        if rc == 0:
            self.elements = int(elements)
        return rc == 0

    def map(self):
        """Blocking device->host copy; returns a float32 view (elements x stride/4) or None."""
        p = lib().rt_array_map(self._h)
        if not p:
            return None
        n = self.elements * self.stride // 4
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n,)).reshape(self.elements, -1)

    def unmap(self):
        check(lib().rt_array_unmap(self._h), "unmap")

    def write(self, data):
        a = np.ascontiguousarray(data)
        if a.nbytes < self.elements * self.stride:
            raise ValueError("array write smaller than the array")
        return lib().rt_array_write(self._h, a.ctypes.data) == 0

    def device_pointer(self):
        return lib().rt_array_device_pointer(self._h)


class Texture:
    """ITexture over a device allocation."""

    def __init__(self, device):
        h = C.c_void_p()
        check(lib().rt_texture_create(device._h, C.byref(h)), "texture_create")
        self._h = h.value
        self._device = device

    def create(self, dimensions, fmt, width, height, data, binding=0, cpu_flags=0):
        a = np.ascontiguousarray(data)
        return lib().rt_texture_init(self._h, dimensions, fmt, width, height, a.ctypes.data, binding, cpu_flags) == 0

    def __del__(self):
        try:
            if self._h and self._device._h:   # a destroyed device already freed its textures
                lib().rt_texture_destroy(self._h)
        except Exception:
            pass


class Compute:
    """ICompute (Factories/ICompute.h:16-59)."""

    def __init__(self, device):
        self.device = device
        h = C.c_void_p()
        check(lib().rt_compute_create(device._h, C.byref(h)), "compute_create")
        self._h = h.value
        self.thread_size = (0, 0, 0)

    def create(self, directory, file_name, main, thread_size, macros=()):
        names = (C.c_char_p * max(1, len(macros)))(*[k.encode() for k, _ in macros])
        vals = (C.c_char_p * max(1, len(macros)))(*[str(v).encode() for _, v in macros])
        tx, ty, tz = thread_size
        rc = lib().rt_compute_load(self._h, directory.encode(), file_name.encode(), main.encode(), tx, ty, tz,
                                   names, vals, len(macros))
        if rc == 0:
            self.thread_size = (tx, ty, tz)
        return rc == 0

    def swap(self):
        return lib().rt_compute_swap(self._h) == 1

    def run(self, dx, dy, dz=1):
        check(lib().rt_compute_run(self._h, dx, dy, dz), "run")

    def get_variable(self, name):
        h = lib().rt_compute_get_variable(self._h, name.encode())
        return ShaderVariable(h, self) if h else None

    def get_array(self, name):
        h = lib().rt_compute_get_array(self._h, name.encode())
        return ShaderArray(h, self) if h else None

    def get_buffer(self, name):
        return None  # the reference's getBuffer always returns nullptr (ComputeDirect3D.cpp:138-141)

    def set_texture(self, stage, texture):
        check(lib().rt_compute_set_texture(self._h, stage, texture._h if texture else None), "set_texture")

    def get_thread_size(self):
        return self.thread_size

    def __del__(self):
        try:
            if self._h and self.device._h:    # a destroyed device already freed its computes
                lib().rt_compute_destroy(self._h)
        except Exception:
            pass


class Device:
    """IDevice over rt_device (DeviceDirect3D's role)."""

    def __init__(self, width, height, gpu=0, float_output=False, stats=False, graph=False, small_rings=False,
                 debug_withhold_fuse=False, gated=False, debug_gate_stress=False, deferred=False,
                 debug_defer_small=False):
        """small_rings: diagnostic RT_DEVICE_DEBUG_SMALL_RINGS (k_trace's LDS long-ray ring holds 64
        entries and its fin pool 8 slots, so queued long rays take the per-block spill rings and long
        shadows the fin[t] fallback; same bits).  debug_withhold_fuse: diagnostic
        RT_DEVICE_DEBUG_WITHHOLD_FUSE (a trace this device leads runs none of the next batch's fused
        prepass tasks, so that batch's wait times out: the fail-safe's test).  gated:
        RT_DEVICE_GATED (the gated launch: the prepass inside the trace kernel instead of its own launch
        before it; same bits, measured slower).  deferred: RT_DEVICE_DEFERRED (ABI 9; a render's trace
        launches with the next render, which runs its own frame's prepass inside that trace kernel; every
        other call that launches on or reads the device launches a pending frame first; one frame to a launch, a
        device under 1280x720 pixels renders as without it).  debug_defer_small: diagnostic
        RT_DEVICE_DEBUG_DEFER_SMALL (the one-frame deferral at every size, for tests on small frames)."""
        self.width, self.height, self.gpu = int(width), int(height), int(gpu)
        self.flags = ((_native.RT_DEVICE_FLOAT_OUTPUT if float_output else 0) | (_native.RT_DEVICE_STATS if stats else 0)
                      | (_native.RT_DEVICE_GRAPH if graph else 0)
                      | (_native.RT_DEVICE_DEBUG_SMALL_RINGS if small_rings else 0)
                      | (_native.RT_DEVICE_DEBUG_WITHHOLD_FUSE if debug_withhold_fuse else 0)
                      | (_native.RT_DEVICE_GATED if gated else 0)
                      | (_native.RT_DEVICE_DEBUG_GATE_STRESS if debug_gate_stress else 0)
                      | (_native.RT_DEVICE_DEFERRED if deferred else 0)
                      | (_native.RT_DEVICE_DEBUG_DEFER_SMALL if debug_defer_small else 0))
        self._h = None

    def create(self):
        h = C.c_void_p()
        rc = lib().rt_device_create(self.gpu, self.width, self.height, self.flags, C.byref(h))
        if rc != 0:
            return False
        self._h = h.value
        return True

    def present(self):
        check(lib().rt_device_present(self._h), "present")

    def flush(self):
        check(lib().rt_device_flush(self._h), "flush")

    def synchronize(self):
        check(lib().rt_device_synchronize(self._h), "synchronize")

    def create_compute(self):
        return Compute(self)

    def create_texture(self):
        return Texture(self)

    def readback(self):
        out = np.empty((self.height, self.width, 4), np.uint8)
        check(lib().rt_device_readback(self._h, out.ctypes.data, self.width * 4), "readback")
        return out

    def readback_float(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        check(lib().rt_device_readback_float(self._h, out.ctypes.data), "readback_float")
        return out

    def readback_bgrx(self):
        """The recorder's view of the frame: (H, W) uint32 (B, G, R, 0) rows, swizzled on the GPU
        (DeviceDirect3D.cpp:242-256 + RecorderWinAPI.cpp:244-253)."""
        out = np.empty((self.height, self.width), np.uint32)
        check(lib().rt_device_readback_bgrx(self._h, out.ctypes.data, self.width * 4), "readback_bgrx")
        return out

    def readback_ring(self, format="rgba8", depth=3):
        """rt_readback_create (ABI 9, additive): a ring of `depth` (1..8) asynchronous captures of this device's
        frames, "rgba8" (readback()'s bytes) or "bgrx" (readback_bgrx()'s)."""
        return ReadbackRing(self, format, depth)

    def stats(self, reset=True):
        s = _native.RtStats()
        check(lib().rt_device_stats_sized(self._h, C.byref(s), C.sizeof(s), 1 if reset else 0), "stats")
        return {n: int(getattr(s, n)) for n, _ in s._fields_}

    def launch_info(self):
        """(gated launches, prepass launches) of the renders this device led (rt_device_info, ABI 7): the
        gated launch runs the prepass inside the trace kernel, a prepass launch is the ABI <= 6 sequence."""
        return self._info((0, 1))

    def prestream_renders(self):
        """Renders whose prepass ran on the device's prepass stream, behind the previous frame's k_order
        (rt_terrain_render with a frame in flight; RT_INFO_PRESTREAM_RENDERS)."""
        return self._info((2,))[0]

    def deferred_fused(self):
        """RT_DEVICE_DEFERRED renders whose prepass ran inside the previous frame's trace kernel
        (RT_INFO_DEFERRED_FUSED, ABI 9)."""
        return self._info((3,))[0]

    def defer_batch(self, frames):
        """rt_device_defer_batch (ABI 9, RT_DEVICE_DEFERRED devices): trace `frames` (1..4) frames to a launch, the
        next group's prepasses inside it; a flush launches all queued frames, the last into the device's buffers."""
        check(lib().rt_device_defer_batch(self._h, int(frames)), "defer_batch")

    def reserve_cus(self, n):
        """rt_device_reserve_cus (ABI 8): this device's trace kernels leave n CUs free for other streams'
        kernels (rank 0's RCCL receive at N > 1)."""
        check(lib().rt_device_reserve_cus(self._h, int(n)), "reserve_cus")

    def _info(self, keys):
        out = []
        for key in keys:
            v = C.c_ulonglong()
            check(lib().rt_device_info(self._h, key, C.byref(v)), "device info")
            out.append(int(v.value))
        return tuple(out)

    def graph_info(self):
        """RT_DEVICE_GRAPH: (graphs captured, graph launches) since creation."""
        cap, lau = C.c_ulonglong(), C.c_ulonglong()
        check(lib().rt_device_graph_info(self._h, C.byref(cap), C.byref(lau)), "graph_info")
        return int(cap.value), int(lau.value)

    def wait_event(self, hip_event):
        """rt_device_wait_event (ABI 6): the device's later work waits for `hip_event` (a hipEvent_t
        handle, e.g. torch.cuda.Event.cuda_event recorded after the caller's fills on its stream)."""
        check(lib().rt_device_wait_event(self._h, int(hip_event)), "wait_event")

    def record_event(self, hip_event):
        """rt_device_record_event (ABI 6): record `hip_event` after the device's queued work (the
        caller's stream then waits for it before reading the device's outputs)."""
        check(lib().rt_device_record_event(self._h, int(hip_event)), "record_event")

    def check(self):
        """rt_device_check (ABI 6): synchronise and raise NativeError if a k_trace queue push was
        dropped at its bound since the last check (never expected: rt_spill_caps)."""
        check(lib().rt_device_check(self._h), "device check")

    def framebuffer_pointer(self):
        return lib().rt_device_framebuffer(self._h)

    def stream(self):
        return lib().rt_device_stream(self._h)

    def set_stream(self, stream_ptr):
        check(lib().rt_device_set_stream(self._h, stream_ptr), "set_stream")

    def destroy(self):
        if self._h:
            lib().rt_device_destroy(self._h)
            self._h = None


class ReadbackRing:
    """rt_readback_* (ABI 9, additive): frames handed to the host without a host synchronisation per frame.
    submit() captures the latest render's frame and returns its ticket without waiting for the GPU (on a
    deferred device without launching the pending frame); wait(t) returns the capture's pinned slot as a
    read-only array, valid until release(t)."""

    FORMATS = {"rgba8": _native.RT_READBACK_RGBA8, "bgrx": _native.RT_READBACK_BGRX}

    def __init__(self, device, format="rgba8", depth=3):
        if format not in self.FORMATS:
            raise ValueError(f"readback ring format {format!r}: 'rgba8' or 'bgrx'")
        self.device, self.format, self.depth = device, format, int(depth)
        h = C.c_void_p()
        check(lib().rt_readback_create(device._h, self.FORMATS[format], self.depth, C.byref(h)), "readback ring")
        self._h = h.value

    def submit(self):
        t = C.c_ulonglong()
        check(lib().rt_readback_submit(self._h, C.byref(t)), "readback submit")
        return int(t.value)

    def ready(self, ticket):
        """True once the capture is in its pinned slot; launches nothing."""
        rc = lib().rt_readback_ready(self._h, int(ticket))
        if rc < 0:
            check(rc, "readback ready")
        return rc == 1

    def wait(self, ticket):
        """(H, W, 4) uint8 ("rgba8") or (H, W) uint32 ("bgrx"): a read-only view of the pinned slot."""
        p = C.c_void_p()
        check(lib().rt_readback_wait(self._h, int(ticket), C.byref(p)), "readback wait")
        w, h = self.device.width, self.device.height
        buf = (C.c_ubyte * (w * h * 4)).from_address(p.value)
        a = np.frombuffer(buf, np.uint8).reshape(h, w, 4) if self.format == "rgba8" else \
            np.frombuffer(buf, np.uint32).reshape(h, w)
        a.flags.writeable = False
        return a

    def release(self, ticket):
        check(lib().rt_readback_release(self._h, int(ticket)), "readback release")

    def destroy(self):
        if self._h:
            lib().rt_readback_destroy(self._h)
            self._h = None


class DeviceFactory:
    @staticmethod
    def construct(api, width, height, gpu=0, **kw):
        """DeviceFactory::construct (DeviceFactory.cpp:6-29): nullptr (None) on failure."""
        if api != DeviceAPI.HIP:
            return None
        d = Device(width, height, gpu, **kw)
        return d if d.create() else None


class Recorder:
    """IRecorder / RecorderWinAPI (Factories/IRecorder.h, Adapters/RecorderWinAPI.cpp) over the
    raw-video sink of rt_recorder_create: frames as raw (B, G, R, 0) rows in `path`, sample time
    stamps in `path`.txt.  Attached to its device: Device.present() writes each frame while
    recording, as DeviceDirect3D::present does."""

    def __init__(self, handle, device, path):
        self._h, self.device, self.path = handle, device, path

    def start(self):
        check(lib().rt_recorder_start(self._h), "recorder start")

    def stop(self):
        check(lib().rt_recorder_stop(self._h), "recorder stop")

    def is_recording(self):
        return lib().rt_recorder_is_recording(self._h) == 1

    def set_frame_time(self, seconds):
        """Timer::getConstant() of the next frame (used when not fixed speed)."""
        check(lib().rt_recorder_set_frame_time(self._h, float(seconds)), "recorder frame time")

    def write(self, frame, stride=None):
        """IRecorder::write(frame, stride) with host RGBA8 rows (an (H, W, 4) uint8 array)."""
        a = np.ascontiguousarray(frame)
        check(lib().rt_recorder_write(self._h, a.ctypes.data, int(stride or a.strides[0])), "recorder write")

    def set_async(self, depth):
        """rt_recorder_set_async (ABI 9, additive): depth 1..8 = a recording present() submits the frame to a BGRX
        readback ring and writes the older frames that are ready, instead of waiting for the frame; 0 = synchronous
        (the default).  stop(), info(), destroy() and this call write everything captured first; same files."""
        check(lib().rt_recorder_set_async(self._h, int(depth)), "recorder set_async")

    def info(self):
        f, t, d = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        check(lib().rt_recorder_info(self._h, C.byref(f), C.byref(t), C.byref(d)), "recorder info")
        return {"frames": f.value, "next_sample_time": t.value, "frame_duration": d.value}

    def destroy(self):
        if self._h:
            lib().rt_recorder_destroy(self._h)
            self._h = None


class RecorderFactory:
    @staticmethod
    def construct(device, frame_rate, fixed_speed, path="output.rgb32", async_depth=0):
        """RecorderFactory::construct (RecorderFactory.cpp:6-19): None on failure.  async_depth > 0: the
        pipelined recorder (Recorder.set_async)."""
        h = C.c_void_p()
        if lib().rt_recorder_create(device._h, int(frame_rate), 1 if fixed_speed else 0, path.encode(), C.byref(h)):
            return None
        if async_depth and lib().rt_recorder_set_async(h.value, int(async_depth)):
            lib().rt_recorder_destroy(h.value)
            return None
        return Recorder(h.value, device, path)


def read_recording(path, width, height):
    """(frames (F, H, W) uint32 BGRX, samples (F, 3) uint64 [frame, time, duration]) of a recording."""
    raw = np.fromfile(path, np.uint32)
    frames = raw.reshape(-1, height, width)
    rows = [ln.split() for ln in open(path + ".txt") if ln.strip() and not ln.startswith("#")]
    return frames, np.array(rows, np.uint64).reshape(-1, 3)


class VariableManager:
    """Common/VariableManager (the live-tweak TCP server, main.cpp:99 `-m`), native in the runtime:
    start() serves the protocol of varclient.VariableClient on a thread."""

    @staticmethod
    def start(port=10666, bind_address="127.0.0.1"):
        check(lib().rt_varmgr_start(int(port), bind_address.encode()), "variable manager start")

    @staticmethod
    def stop():
        check(lib().rt_varmgr_stop(), "variable manager stop")

    @staticmethod
    def count():
        return int(lib().rt_varmgr_count())

    @staticmethod
    def register_compute(compute):
        check(lib().rt_varmgr_register_compute(compute._h), "variable manager register")


class Noise:
    """Graphics/Noise.cpp:39-94 via rt_noise_generate (seed 300 unless random)."""
    TEXTURE_SIZE = 128
    RAND_MSVC, RAND_GLIBC = 0, 1

    def __init__(self):
        self.permutations2D = None
        self.permutations1D = None

    def generate(self, random=False, seed=None, rand_kind=RAND_MSVC):
        import time
        if seed is None:
            seed = int(time.time()) & 0xFFFFFFFF if random else 300
        p2 = np.empty(128 * 128 * 4, np.uint8)
        g = np.empty(128 * 4, np.float32)
        check(lib().rt_noise_generate(seed, rand_kind, p2.ctypes.data, g.ctypes.data), "noise_generate")
        self.permutations2D, self.permutations1D = p2, g


def set_target_depths_host(camera_results):
    cr = np.ascontiguousarray(camera_results, np.float32).reshape(1024, 4)
    cd = np.empty((1024, 2), np.float32)
    check(lib().rt_terrain_set_target_depths(cr.ctypes.data, cd.ctypes.data), "set_target_depths")
    return cd


class Terrain:
    """Graphics/Terrain.{h,cpp}: creates the two computes, binds variables by name after
    swap, and renders a frame.  render() keeps the reference's call sequence (prepass ->
    CameraResults map/unmap -> host setTargetDepths -> CellDistance write -> tiled runs);
    render_device() is the same frame with the round trip kept on the GPU."""

    def __init__(self, device, theme="nomadplains", record_mode=False, aa_samples=1, max_steps=0,
                 noise_seed=300, rand_kind=Noise.RAND_MSVC, ao_samples=0):
        vfs_add_path("Media/" + theme)  # Terrain.cpp:23
        self.device, self.theme, self.record_mode = device, theme, record_mode
        # max_steps / ao_samples: build extensions (BASELINE configs), 0 = reference semantics
        self.aa_samples, self.max_steps, self.ao_samples = aa_samples, max_steps, ao_samples
        self.noise_seed, self.rand_kind = noise_seed, rand_kind
        self.compute = self.camera_compute = None
        self.camera = None
        self.camera_view = np.zeros((CAMERA_VIEW_RES * CAMERA_VIEW_RES, 4), np.float32)
        self.sun = np.zeros(3, np.float32)

    def create(self):  # Terrain.cpp:69-89
        self.calculate_tile_sizes()
        self.compute = self.device.create_compute()
        self.camera_compute = self.device.create_compute()
        self.noise = Noise()
        self.noise.generate(seed=self.noise_seed, rand_kind=self.rand_kind)
        self.tex_noise_2d = self.device.create_texture()
        ok = self.tex_noise_2d.create(_native.RT_TEXTURE_2D, _native.RT_FORMAT_R8G8B8A8_UINT, 128, 128,
                                      self.noise.permutations2D)
        if not ok:
            raise RuntimeError("texture create failed: " + lib().rt_last_error().decode())

    def reload(self):  # Terrain.cpp:91-103
        macros = [("RECORDING", "1")] if self.record_mode else []
        if self.aa_samples != 1:
            macros.append(("AA_SAMPLES", str(self.aa_samples)))
        if self.max_steps:
            macros.append(("RT_MAX_STEPS", str(self.max_steps)))
        screen_macros = macros + ([("RT_AO_SAMPLES", str(self.ao_samples))] if self.ao_samples else [])
        ok1 = self.compute.create("shaders", "tracescreen.hlsl", "CSMain", (self.thread_x, self.thread_y, 1),
                                  screen_macros)
        ok2 = self.camera_compute.create("shaders", "camerarays.hlsl", "CSMain",
                                         (CAMERA_THREAD_RES, CAMERA_THREAD_RES, 1), macros)
        return ok1 and ok2

    def calculate_tile_sizes(self):  # Terrain.cpp:208-242
        resx, resy = self.device.width, self.device.height
        divisor = 4 if self.record_mode else 1
        tpx, tpy = 1024 // divisor, 512 // divisor
        self.tiles_x = -(-resx // tpx)
        self.tiles_y = -(-resy // tpy)
        self.tile_x, self.tile_y = resx // self.tiles_x, resy // self.tiles_y
        self.thread_x = self.thread_y = 16
        while self.tile_x % self.thread_x:
            self.thread_x += 1
        while self.tile_y % self.thread_y:
            self.thread_y += 1
        self.dispatch_x, self.dispatch_y = self.tile_x // self.thread_x, self.tile_y // self.thread_y

    def set_camera(self, camera):
        self.camera = camera

    def update_shaders(self):  # Terrain.cpp:138-206
        cam = self.camera
        proj = _cbuffer_matrix(cam.projection_hlsl())
        screen = np.array([cam.width, cam.height], np.float32)
        if self.compute.swap():
            self.var_view = self.compute.get_variable("ViewInverse")
            self.var_eye = self.compute.get_variable("Eye")
            self.var_sun = self.compute.get_variable("SunDirection")
            self.var_thread_offset = self.compute.get_variable("ThreadOffset")
            self.var_cell_distance = self.compute.get_array("CellDistance")
            if self.var_cell_distance:
                self.var_cell_distance.create(CAMERA_VIEW_RES * CAMERA_VIEW_RES)
            for name, val in (("Projection", proj), ("ScreenSize", screen), ("permGradients", self.noise.permutations1D)):
                v = self.compute.get_variable(name)
                if v:
                    v.write(val)
            self.compute.set_texture(0, self.tex_noise_2d)
            self._write_frame_vars()
        if self.camera_compute.swap():
            self.var_cam_view = self.camera_compute.get_variable("ViewInverse")
            self.var_cam_eye = self.camera_compute.get_variable("Eye")
            self.var_cam_results = self.camera_compute.get_array("CameraResults")
            if self.var_cam_results:
                self.var_cam_results.create(CAMERA_VIEW_RES * CAMERA_VIEW_RES)
            for name, val in (("Projection", proj), ("ScreenSize", screen), ("permGradients", self.noise.permutations1D)):
                v = self.camera_compute.get_variable(name)
                if v:
                    v.write(val)
            self.camera_compute.set_texture(0, self.tex_noise_2d)
            self._write_frame_vars()

    def _write_frame_vars(self):
        """Variables set before the first dispatch (avoids the frame-1 zero-constant
        artefact of the reference)."""
        if self.camera is None:
            return
        self.update_terrain()
        self.set_time_of_day_vec(self.sun)

    def update_terrain(self, time=0.0):  # Terrain.cpp:302-311
        vinv = _cbuffer_matrix(self.camera.view_inverse_hlsl())
        eye = self.camera.eye()
        for v in (getattr(self, "var_view", None), getattr(self, "var_cam_view", None)):
            if v:
                v.write(vinv)
        for v in (getattr(self, "var_eye", None), getattr(self, "var_cam_eye", None)):
            if v:
                v.write(eye)

    def set_time_of_day(self, time_of_day):  # Terrain.cpp:285-300
        from .camera import sun_direction
        self.set_time_of_day_vec(sun_direction(time_of_day))

    def set_time_of_day_vec(self, sun):
        self.sun = np.asarray(sun, np.float32)
        v = getattr(self, "var_sun", None)
        if v:
            v.write(self.sun)

    def get_camera_results(self):  # Terrain.cpp:441-452
        fd = self.var_cam_results.map()
        if fd is None:
            return
        self.camera_view[:] = fd
        self.var_cam_results.unmap()
        if self.var_cell_distance:
            self.var_cell_distance.write(set_target_depths_host(self.camera_view))

    def render(self):  # Terrain.cpp:105-136 (reference call sequence)
        self.update_shaders()
        n = -(-CAMERA_VIEW_RES // CAMERA_THREAD_RES)
        self.camera_compute.run(n, n, 1)
        self.get_camera_results()
        if self.var_thread_offset:
            for x in range(self.tiles_x):
                for y in range(self.tiles_y):
                    off = np.array([x * self.dispatch_x * self.thread_x, y * self.dispatch_y * self.thread_y], np.uint32)
                    self.var_thread_offset.write(off)
                    self.compute.run(self.dispatch_x, self.dispatch_y, 1)
                    self.device.flush()
        else:
            self.compute.run(self.dispatch_x * self.tiles_x, self.dispatch_y * self.tiles_y, 1)

    def render_device(self, shard_rank=0, shard_count=1, feed=False):
        """Terrain::render with setTargetDepths on the GPU: no host round trip, all on one stream.
        feed=True also sends this frame's CameraResults to the host right after the prepass
        (camera_feed() collects them) -- what Flyby reads, without waiting for the whole frame."""
        self.update_shaders()
        fn = lib().rt_terrain_render_feed if feed else lib().rt_terrain_render
        check(fn(self.camera_compute._h, self.compute._h, shard_rank, shard_count), "terrain_render")

    def camera_feed(self):
        """Wait for the feed of the last render_device(feed=True); it becomes the camera view
        (Terrain::getCameraView, Terrain.cpp:441-452) and is returned, (1024, 4) float32."""
        out = np.empty((CAMERA_VIEW_RES * CAMERA_VIEW_RES, 4), np.float32)
        check(lib().rt_terrain_feed_wait(self.camera_compute._h, out.ctypes.data), "camera feed")
        self.camera_view[:] = out
        return self.camera_view

    def trace_rays(self, origins, dirs, eye=None, steps=False, mode="auto", max_blocks=0):
        """rt_terrain_trace_rays: what n rays of the caller's own hit, marched as the prepass marches its
        pixel rays (camerarays.hlsl:12-21).  origins, dirs: (n, 3); dirs are used as given (their length enters
        the first step).  eye: the level-of-detail eye (default: the camera's, the compute's current Eye).
        Returns results (n, 4) float32 -- the last sample's position and the hit distance, 5000 for a miss --
        or (results, steps) with the march loops' iteration counts (n,) uint32; None if the call fails
        (lib().rt_last_error()).  mode: "auto", "segments" (nomadplains only) or "lanes"; max_blocks caps the
        lanes shape's persistent grid.  Blocking; uses the camerarays compute; needs set_camera() first."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("trace_rays: %d origins, %d dirs" % (len(o), len(d)))
        n = len(o)
        opt = ray_options(eye, mode, max_blocks)
        self.update_shaders()
        res = np.empty((n, 4), np.float32)
        st = np.empty(n, np.uint32) if steps else None
        rc = lib().rt_terrain_trace_rays(self.camera_compute._h, o.ctypes.data, d.ctypes.data, n, C.byref(opt),
                                         res.ctypes.data, st.ctypes.data if steps else None)
        if rc != _native.RT_OK:
            return None
        return (res, st) if steps else res

    def trace_rays_device(self, rays_ptr, n, results_ptr, steps_ptr=0, eye=None, mode="auto", max_blocks=0):
        """rt_terrain_trace_rays_device: the same for device arrays -- rays_ptr n x 8 float32 (pack_rays'
        layout), results_ptr n x 4 float32, steps_ptr n uint32 or 0 -- enqueued on the device's stream with no
        host synchronisation (order other streams with Device.wait_event / record_event).  True on success."""
        opt = ray_options(eye, mode, max_blocks)
        self.update_shaders()
        rc = lib().rt_terrain_trace_rays_device(self.camera_compute._h, rays_ptr or None, int(n), C.byref(opt),
                                                results_ptr or None, steps_ptr or None)
        return rc == _native.RT_OK

    def trace_surface(self, origins, dirs, ranges=None, eye=None, t_min=None, t_max=None, stepmod=None, max_steps=0,
                      steps=False, mode="auto", max_blocks=0):
        """rt_terrain_trace_surface: where n rays of the caller's own meet the surface and its normal there --
        the refined march tracescreen runs for its pixels (tracing.hlsl:47-105, skiprefine off) and getNormal
        (:107-116).  origins, dirs: (n, 3), dirs used as given; ranges: (n, 2) t_min_i, t_max_i per ray, or None
        for t_min / t_max (defaults 0.01 and 5000); stepmod default 1; max_steps 0 is unbounded, and a ray whose
        step count equals a cap may be mid-refinement.  eye: the LOD eye and getNormal's (default: the camera's).
        Returns results (n, 8) float32 -- last sample xyz, distance | unit normal, density; a hit is
        results[:, 7] > 0 and a miss has a zero normal -- or (results, steps); None if the call fails
        (lib().rt_last_error()).  mode, max_blocks: as trace_rays.  Blocking; needs set_camera() first."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("trace_surface: %d origins, %d dirs" % (len(o), len(d)))
        n = len(o)
        rg = None
        if ranges is not None:
            rg = np.ascontiguousarray(ranges, np.float32).reshape(-1, 2)
            if len(rg) != n:
                raise ValueError("trace_surface: %d rays, %d ranges" % (n, len(rg)))
        opt = surface_options(eye, mode, max_blocks, t_min, t_max, stepmod, max_steps)
        self.update_shaders()
        res = np.empty((n, 8), np.float32)
        st = np.empty(n, np.uint32) if steps else None
        rc = lib().rt_terrain_trace_surface(self.camera_compute._h, o.ctypes.data, d.ctypes.data,
                                            rg.ctypes.data if rg is not None else None, n, C.byref(opt),
                                            res.ctypes.data, st.ctypes.data if steps else None)
        if rc != _native.RT_OK:
            return None
        return (res, st) if steps else res

    def trace_surface_device(self, rays_ptr, n, results_ptr, steps_ptr=0, ray_range=False, eye=None, t_min=None,
                             t_max=None, stepmod=None, max_steps=0, mode="auto", max_blocks=0):
        """rt_terrain_trace_surface_device: the same for device arrays -- rays_ptr n x 8 float32 (pack_rays'
        layout; with ray_range its spare words are the rays' ranges), results_ptr n x 8 float32, steps_ptr n
        uint32 or 0 -- enqueued on the device's stream with no host synchronisation.  True on success."""
        opt = surface_options(eye, mode, max_blocks, t_min, t_max, stepmod, max_steps, ray_range)
        self.update_shaders()
        rc = lib().rt_terrain_trace_surface_device(self.camera_compute._h, rays_ptr or None, int(n), C.byref(opt),
                                                   results_ptr or None, steps_ptr or None)
        return rc == _native.RT_OK

    def shade_rays(self, origins, dirs, ranges=None, eye=None, t_min=None, t_max=None, stepmod=None, max_steps=0,
                   rgba8=False, steps=False, max_blocks=0):
        """rt_terrain_shade_rays: what n rays of the caller's own LOOK like -- the sample tracescreen computes for
        a pixel ray (tracescreen.hlsl:16-48): terrain colour with the sun's shadow, fog and sky, or the sky for a
        miss.  One sample per ray and NO ambient occlusion, whatever the Terrain was built with.  origins, dirs,
        ranges, t_min, t_max, stepmod, max_steps: as trace_surface.  eye: the density's LOD eye, getNormal's and
        the sky's (default: the camera's).  The sun is the Terrain's (set_time_of_day).
        Returns results (n, 8) float32 -- colour rgb (not saturated), distance | last sample xyz, density; a hit
        is results[:, 7] > 0 -- or a tuple (results, [pixels (n,) uint32 RGBA8, R in the low byte, alpha 255, if
        rgba8], [steps (n, 2) uint32: primary and shadow iterations, if steps]); None if the call fails
        (lib().rt_last_error()).  max_blocks caps the persistent grid.  Blocking; uses the tracescreen compute;
        needs set_camera() first."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("shade_rays: %d origins, %d dirs" % (len(o), len(d)))
        n = len(o)
        rg = None
        if ranges is not None:
            rg = np.ascontiguousarray(ranges, np.float32).reshape(-1, 2)
            if len(rg) != n:
                raise ValueError("shade_rays: %d rays, %d ranges" % (n, len(rg)))
        opt = surface_options(eye, "auto", max_blocks, t_min, t_max, stepmod, max_steps)
        self.update_shaders()
        res = np.empty((n, 8), np.float32)
        px = np.empty(n, np.uint32) if rgba8 else None
        st = np.empty((n, 2), np.uint32) if steps else None
        rc = lib().rt_terrain_shade_rays(self.compute._h, o.ctypes.data, d.ctypes.data,
                                         rg.ctypes.data if rg is not None else None, n, C.byref(opt), res.ctypes.data,
                                         px.ctypes.data if rgba8 else None, st.ctypes.data if steps else None)
        if rc != _native.RT_OK:
            return None
        out = (res,) + ((px,) if rgba8 else ()) + ((st,) if steps else ())
        return out if len(out) > 1 else res

    def shade_rays_device(self, rays_ptr, n, results_ptr=0, rgba8_ptr=0, steps_ptr=0, ray_range=False, eye=None,
                          t_min=None, t_max=None, stepmod=None, max_steps=0, max_blocks=0):
        """rt_terrain_shade_rays_device: the same for device arrays -- rays_ptr n x 8 float32 (pack_rays' layout;
        with ray_range its spare words are the rays' ranges), results_ptr n x 8 float32 or 0, rgba8_ptr n uint32
        or 0 (one of the two at least), steps_ptr n x 2 uint32 or 0 -- enqueued on the device's stream with no
        host synchronisation.  True on success."""
        opt = surface_options(eye, "auto", max_blocks, t_min, t_max, stepmod, max_steps, ray_range)
        self.update_shaders()
        rc = lib().rt_terrain_shade_rays_device(self.compute._h, rays_ptr or None, int(n), C.byref(opt),
                                                results_ptr or None, rgba8_ptr or None, steps_ptr or None)
        return rc == _native.RT_OK

    def shade_points(self, points, normals, eye=None, ao_samples=0, seed=0, rgba8=False, steps=False, max_blocks=0):
        """rt_terrain_shade_points: what the terrain LOOKS like at n points the caller already holds -- getColor
        with the sun's shadow ray, and the AO factor of ao_samples (0..16) hemisphere rays about the normal --
        exactly as a frame computes both for a pixel whose primary ray ended there, without the view ray's fog and
        sky blends.  points: (n, 3), or (n, 4) rows x y z _ (extract_mesh_device's vertices); normals: (n, 3), or
        (n, 4) rows nx ny nz _ (sample_field(normals=True), extract_mesh's normals), used as given.  eye: the LOD
        eye and the viewpoint of the colour (default: the camera's).  seed: any uint32; the AO directions are a
        hash of (point index, seed, k).  The sun is the Terrain's (set_time_of_day).
        Returns results (n, 4) float32 -- colour rgb (not saturated, not multiplied by ao), ao -- or a tuple
        (results, [pixels (n,) uint32 RGBA8 of ao times the saturated colour, R in the low byte, alpha 255, if
        rgba8], [steps (n, 2) uint32: shadow iterations and the AO rays' sum, if steps]); None if the call fails
        (lib().rt_last_error()).  max_blocks caps the persistent grid.  Blocking; uses the tracescreen compute;
        needs set_camera() first."""
        p, nr = _xyz_rows(points), _xyz_rows(normals)
        if len(p) != len(nr):
            raise ValueError("shade_points: %d points, %d normals" % (len(p), len(nr)))
        n = len(p)
        opt = point_options(eye, ao_samples, seed, max_blocks)
        self.update_shaders()
        res = np.empty((n, 4), np.float32)
        px = np.empty(n, np.uint32) if rgba8 else None
        st = np.empty((n, 2), np.uint32) if steps else None
        rc = lib().rt_terrain_shade_points(self.compute._h, p.ctypes.data, nr.ctypes.data, n, C.byref(opt),
                                           res.ctypes.data, px.ctypes.data if rgba8 else None,
                                           st.ctypes.data if steps else None)
        if rc != _native.RT_OK:
            return None
        out = (res,) + ((px,) if rgba8 else ()) + ((st,) if steps else ())
        return out if len(out) > 1 else res

    def shade_points_device(self, points_ptr, normals_ptr, n, results_ptr=0, rgba8_ptr=0, steps_ptr=0, eye=None,
                            ao_samples=0, seed=0, max_blocks=0):
        """rt_terrain_shade_points_device: the same for device arrays -- points_ptr and normals_ptr n x 4 float32
        (x y z _ and nx ny nz _, the spare words ignored: extract_mesh_device's vertices and normals as they are),
        results_ptr n x 4 float32 or 0, rgba8_ptr n uint32 or 0 (one of the two at least), steps_ptr n x 2 uint32
        or 0; points, normals and results 16-byte aligned -- enqueued on the device's stream with no host
        synchronisation.  True on success."""
        opt = point_options(eye, ao_samples, seed, max_blocks)
        self.update_shaders()
        rc = lib().rt_terrain_shade_points_device(self.compute._h, points_ptr or None, normals_ptr or None, int(n),
                                                  C.byref(opt), results_ptr or None, rgba8_ptr or None,
                                                  steps_ptr or None)
        return rc == _native.RT_OK

    def sample_field(self, points, eye=None, normals=False, max_blocks=0):
        """rt_terrain_sample_field: what the terrain IS at n points -- the density getDensity gives (> 0 inside),
        and with normals getNormal (tracing.hlsl:107-116) there too, for every point, inside or outside.
        points: (n, 3).  eye: the level-of-detail eye and getNormal's (default: the camera's, the compute's
        current Eye).  Returns (n,) float32 densities, or with normals (n, 4) float32 rows normal xyz, density;
        None if the call fails (lib().rt_last_error()).  max_blocks caps the grid.  Blocking; uses the camerarays
        compute; needs set_camera() first."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = len(p)
        opt = field_options(eye, normals, max_blocks)
        self.update_shaders()
        res = np.empty((n, 4) if normals else n, np.float32)
        rc = lib().rt_terrain_sample_field(self.camera_compute._h, p.ctypes.data, n, C.byref(opt), res.ctypes.data)
        return res if rc == _native.RT_OK else None

    def sample_field_device(self, points_ptr, n, results_ptr, eye=None, normals=False, max_blocks=0):
        """rt_terrain_sample_field_device: the same for device arrays -- points_ptr n x 4 float32 (pack_points'
        layout: x y z _), results_ptr n float32 or with normals n x 4 float32, both 16-byte aligned -- enqueued on
        the device's stream with no host synchronisation.  True on success."""
        opt = field_options(eye, normals, max_blocks)
        self.update_shaders()
        rc = lib().rt_terrain_sample_field_device(self.camera_compute._h, points_ptr or None, int(n), C.byref(opt),
                                                  results_ptr or None)
        return rc == _native.RT_OK

    def sample_lattice(self, origin, spacing, dims, eye=None, normals=False, occupancy=False, max_blocks=0):
        """rt_terrain_sample_lattice: sample_field over the lattice of dims = (nx, ny, nz) points whose point
        (ix, iy, iz) lies at fmaf(i, spacing, origin) per axis (one rounding), computed on the device: no
        coordinates are uploaded.  Returns an array shaped (nz, ny, nx) float32, or (nz, ny, nx, 4) with normals
        (normal xyz, density); with occupancy a tuple of it and the bit words (nz, ny, ceil(nx / 32)) uint32, bit
        ix % 32 of word ix // 32 set where the density is > 0.  None if the call fails."""
        lat, (nx, ny, nz) = lattice(origin, spacing, dims), (int(v) for v in dims)
        opt = field_options(eye, normals, max_blocks)
        self.update_shaders()
        res = np.empty((nz, ny, nx, 4) if normals else (nz, ny, nx), np.float32)
        occ = np.empty((nz, ny, (nx + 31) // 32), np.uint32) if occupancy else None
        rc = lib().rt_terrain_sample_lattice(self.camera_compute._h, C.byref(lat), C.byref(opt), res.ctypes.data,
                                             occ.ctypes.data if occupancy else None)
        if rc != _native.RT_OK:
            return None
        return (res, occ) if occupancy else res

    def sample_lattice_device(self, origin, spacing, dims, results_ptr=0, occupancy_ptr=0, eye=None, normals=False,
                              max_blocks=0):
        """rt_terrain_sample_lattice_device: the same into device arrays -- results_ptr nx ny nz float32 (x 4 with
        normals, 16-byte aligned) or 0, occupancy_ptr ceil(nx / 32) ny nz uint32 or 0 (one of the two at least)
        -- enqueued on the device's stream with no host synchronisation.  True on success."""
        lat = lattice(origin, spacing, dims)
        opt = field_options(eye, normals, max_blocks)
        self.update_shaders()
        rc = lib().rt_terrain_sample_lattice_device(self.camera_compute._h, C.byref(lat), C.byref(opt),
                                                    results_ptr or None, occupancy_ptr or None)
        return rc == _native.RT_OK

    def extract_mesh(self, origin, spacing, dims, eye=None, normals=True, max_blocks=0, colors=False, ao_samples=0,
                     seed=0):
        """rt_terrain_extract_mesh: the terrain's surface inside the lattice (sample_lattice's origin, spacing and
        dims) as a surface-nets triangle mesh, extracted on the device.  Returns (vertices (nv, 3) float32,
        normals (nv, 4) float32 rows getNormal xyz, density -- or None without normals --, triangles (nt, 3) uint32
        wound so that their normals point out of the terrain, cells (nv,) uint32: each vertex's cell index
        (cz (ny - 1) + cy) (nx - 1) + cx); None if a call fails.  Two calls: one that counts and one of the exact
        size, so the lattice's density is computed twice; keep the arrays on the device and size them yourself
        (extract_mesh_device) where that matters.  Blocking; uses the camerarays compute.
        colors: one more array at the end, (nv,) uint32 RGBA8 -- shade_points' pixels for the vertices at their
        normals with the same eye, ao_samples and seed (the tracescreen compute); it needs normals."""
        if colors and not normals:
            raise ValueError("extract_mesh: colors=True shades the vertices at their normals; it needs normals=True")
        mesh = self._extract_mesh(origin, spacing, dims, eye, normals, max_blocks)
        if mesh is None or not colors:
            return mesh
        shaded = self.shade_points(mesh[0], mesh[1], eye=eye, ao_samples=ao_samples, seed=seed, rgba8=True,
                                   max_blocks=max_blocks)
        return None if shaded is None else mesh + (shaded[1],)

    def _extract_mesh(self, origin, spacing, dims, eye, normals, max_blocks):
        lat = lattice(origin, spacing, dims)
        opt = field_options(eye, False, max_blocks)
        self.update_shaders()
        counts = np.zeros(2, np.uint32)
        cs = self.camera_compute._h
        if lib().rt_terrain_extract_mesh(cs, C.byref(lat), C.byref(opt), None, None, 0, None, 0,
                                         counts.ctypes.data) != _native.RT_OK:
            return None
        nv, nt = int(counts[0]), int(counts[1])
        verts = np.zeros((nv, 4), np.float32)
        nrm = np.zeros((nv, 4), np.float32) if normals else None
        tris = np.zeros((nt, 3), np.uint32)
        rc = lib().rt_terrain_extract_mesh(cs, C.byref(lat), C.byref(opt), verts.ctypes.data if nv else None,
                                           nrm.ctypes.data if normals and nv else None, nv,
                                           tris.ctypes.data if nt else None, nt, counts.ctypes.data)
        if rc != _native.RT_OK or (int(counts[0]), int(counts[1])) != (nv, nt):
            return None
        return np.ascontiguousarray(verts[:, :3]), nrm, tris, np.ascontiguousarray(verts[:, 3]).view(np.uint32)

    def extract_mesh_device(self, origin, spacing, dims, scratch_ptr, scratch_bytes, vertices_ptr, normals_ptr,
                            max_vertices, triangles_ptr, max_triangles, counts_ptr, eye=None, max_blocks=0):
        """rt_terrain_extract_mesh_device: the same into device arrays -- scratch_ptr at least
        mesh_scratch_bytes(origin, spacing, dims) bytes, vertices_ptr max_vertices x 4 words (x y z, cell index
        bits), normals_ptr the same shape or 0 (no normal pass), triangles_ptr max_triangles x 3 uint32, counts_ptr
        2 uint32 (the full vertex and triangle counts); scratch, vertices and normals 16-byte aligned -- enqueued
        on the device's stream with no host synchronisation and no allocation.  True on success."""
        lat = lattice(origin, spacing, dims)
        opt = field_options(eye, False, max_blocks)
        self.update_shaders()
        rc = lib().rt_terrain_extract_mesh_device(self.camera_compute._h, C.byref(lat), C.byref(opt),
                                                  scratch_ptr or None, int(scratch_bytes), vertices_ptr or None,
                                                  normals_ptr or None, int(max_vertices), triangles_ptr or None,
                                                  int(max_triangles), counts_ptr or None)
        return rc == _native.RT_OK

    def distance_field(self, origin, spacing, dims, eye=None, max_cells=0, occupancy=None, squared=False, max_blocks=0):
        """rt_terrain_distance_field: for every point of the lattice (sample_lattice's origin, spacing and dims) the
        distance to the nearest lattice point of the other state, formed on the device from the occupancy bits: an
        array shaped (nz, ny, nx) float32, sqrt(d2) * |spacing|, positive in free space, negative in the ground,
        +-inf where the lattice has no point of the other state or none within max_cells cells (0: unbounded).  It
        needs |spacing| equal on the three axes and not 0.  squared: the exact uint32 squared distance in cells^2
        instead (RT_DIST_FAR for none), for any spacing.  occupancy: None for the terrain's own, or bit words
        shaped (nz, ny, ceil(nx / 32)) uint32 as sample_lattice returns them (an edited voxel grid); the terrain is
        not evaluated then.  None if the call fails.  Blocking; uses the camerarays compute."""
        lat, (nx, ny, nz) = lattice(origin, spacing, dims), (int(v) for v in dims)
        opt = distance_options(eye, max_cells, max_blocks)
        occ = None
        if occupancy is not None:
            occ = np.ascontiguousarray(occupancy, np.uint32)
            if occ.size != nz * ny * ((nx + 31) // 32):
                raise ValueError("distance_field: occupancy must hold ceil(nx / 32) * ny * nz words")
        self.update_shaders()
        res = np.empty((nz, ny, nx), np.uint32 if squared else np.float32)
        rc = lib().rt_terrain_distance_field(self.camera_compute._h, C.byref(lat), C.byref(opt),
                                             occ.ctypes.data if occ is not None and occ.size else None,
                                             res.ctypes.data if squared else None, None if squared else res.ctypes.data)
        return res if rc == _native.RT_OK else None

    def distance_field_device(self, origin, spacing, dims, scratch_ptr, scratch_bytes, d2_ptr=0, distance_ptr=0,
                              occupancy_ptr=0, eye=None, max_cells=0, max_blocks=0):
        """rt_terrain_distance_field_device: the same into device arrays -- scratch_ptr at least
        distance_scratch_bytes(origin, spacing, dims) bytes, d2_ptr nx ny nz uint32 or 0, distance_ptr nx ny nz
        float32 or 0 (one of the two at least), occupancy_ptr the caller's bit words or 0 for the terrain's own --
        enqueued on the device's stream with no host synchronisation and no allocation.  True on success."""
        lat = lattice(origin, spacing, dims)
        opt = distance_options(eye, max_cells, max_blocks)
        self.update_shaders()
        rc = lib().rt_terrain_distance_field_device(self.camera_compute._h, C.byref(lat), C.byref(opt),
                                                    occupancy_ptr or None, scratch_ptr or None, int(scratch_bytes),
                                                    d2_ptr or None, distance_ptr or None)
        return rc == _native.RT_OK

    def path_field(self, origin, spacing, dims, seeds, eye=None, clearance=0, occupancy=None, max_cost=0, flow=False,
                   max_sweeps=0, max_blocks=0, status=None):
        """rt_terrain_path_field: for every point of the lattice (sample_lattice's origin, spacing and dims) the cost
        of the cheapest path from the seeds through the passable points, an array shaped (nz, ny, nx) uint32 in
        thirds of a cell (a face move 3, an edge move 4, a corner move 5; world length cost * |spacing| / 3),
        RT_PATH_FAR where a point is blocked, unreachable or beyond max_cost (0: unbounded).  seeds: (n, 3) ix, iy,
        iz, or flat point indices.  clearance: passable points are more than that many cells from every blocked
        point.  occupancy: None for the terrain's own, or bit words as sample_lattice returns them.  flow=True:
        (cost, flow), flow uint8 the move code (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) of the first step back to a
        seed, 13 at a seed, RT_PATH_NONE where the cost is far.  max_sweeps 0: until converged.  status: a list
        that receives the four status words.  None if the call fails.  Blocking; uses the camerarays compute."""
        lat, (nx, ny, nz) = lattice(origin, spacing, dims), (int(v) for v in dims)
        opt = path_options(eye, clearance, max_cost, max_sweeps, max_blocks)
        occ = None
        if occupancy is not None:
            occ = np.ascontiguousarray(occupancy, np.uint32)
            if occ.size != nz * ny * ((nx + 31) // 32):
                raise ValueError("path_field: occupancy must hold ceil(nx / 32) * ny * nz words")
        sd = seed_indices(seeds, (nx, ny, nz))
        self.update_shaders()
        cost = np.empty((nz, ny, nx), np.uint32)
        fl = np.empty((nz, ny, nx), np.uint8) if flow else None
        st = np.zeros(4, np.uint32)
        rc = lib().rt_terrain_path_field(self.camera_compute._h, C.byref(lat), C.byref(opt),
                                         occ.ctypes.data if occ is not None and occ.size else None,
                                         sd.ctypes.data if sd.size else None, int(sd.size),
                                         cost.ctypes.data, fl.ctypes.data if flow and fl.size else None, st.ctypes.data)
        if rc != _native.RT_OK:
            return None
        if status is not None:
            status[:] = [int(v) for v in st]
        return (cost, fl) if flow else cost

    def path_field_device(self, origin, spacing, dims, seeds_ptr, n_seeds, scratch_ptr, scratch_bytes, cost_ptr,
                          status_ptr, flow_ptr=0, occupancy_ptr=0, eye=None, clearance=0, max_cost=0, max_sweeps=1,
                          max_blocks=0):
        """rt_terrain_path_field_device: the same into device arrays -- seeds_ptr n_seeds uint32 point indices,
        scratch_ptr at least path_scratch_bytes(origin, spacing, dims, clearance) bytes, cost_ptr nx ny nz uint32,
        status_ptr 4 uint32, flow_ptr nx ny nz uint8 or 0, occupancy_ptr the caller's bit words or 0 for the
        terrain's own -- an initialisation, exactly max_sweeps (1..4096) sweeps and a finish pass enqueued on the
        device's stream with no host synchronisation and no allocation.  True on success."""
        lat = lattice(origin, spacing, dims)
        opt = path_options(eye, clearance, max_cost, max_sweeps, max_blocks)
        self.update_shaders()
        rc = lib().rt_terrain_path_field_device(self.camera_compute._h, C.byref(lat), C.byref(opt), occupancy_ptr or None,
                                                seeds_ptr or None, int(n_seeds), scratch_ptr or None, int(scratch_bytes),
                                                cost_ptr or None, flow_ptr or None, status_ptr or None)
        return rc == _native.RT_OK

    def visibility_field(self, origin, spacing, dims, observers=None, directions=None, eye=None, max_range=0,
                         occupancy=None, max_blocks=0, status=None):
        """rt_terrain_visibility_field: for every point of the lattice (sample_lattice's origin, spacing and dims) the
        observers it has a free line of sight to over the occupancy bits, an array shaped (nz, ny, nx) uint32: bit k
        is set where the point sees observer k.  observers: (n, 3) ix, iy, iz lattice points, which take the low
        bits in order; directions: (m, 3) integer directions towards a light (lattice_direction), which take the
        next bits, set where the point is lit; n + m is 1..32.  The ends of a line are not tested, so a blocked
        surface point that is met first is seen.  max_range: in cells, 0 for unbounded; a point observer farther
        away is not seen, a shadow caster farther away does not count.  occupancy: None for the terrain's own, or
        bit words as sample_lattice returns them.  status: a list that receives the four status words (points with
        a bit set, bits set, valid observers, 0).  None if the call fails.  Blocking; uses the camerarays compute."""
        lat, (nx, ny, nz) = lattice(origin, spacing, dims), (int(v) for v in dims)
        opt = visibility_options(eye, max_range, max_blocks)
        occ = None
        if occupancy is not None:
            occ = np.ascontiguousarray(occupancy, np.uint32)
            if occ.size != nz * ny * ((nx + 31) // 32):
                raise ValueError("visibility_field: occupancy must hold ceil(nx / 32) * ny * nz words")
        ob = pack_observers(observers, directions, (nx, ny, nz))
        self.update_shaders()
        mask = np.empty((nz, ny, nx), np.uint32)
        st = np.zeros(4, np.uint32)
        rc = lib().rt_terrain_visibility_field(self.camera_compute._h, C.byref(lat), C.byref(opt),
                                               occ.ctypes.data if occ is not None and occ.size else None,
                                               ob.ctypes.data, int(ob.shape[0]), mask.ctypes.data, st.ctypes.data)
        if rc != _native.RT_OK:
            return None
        if status is not None:
            status[:] = [int(v) for v in st]
        return mask

    def visibility_field_device(self, origin, spacing, dims, observers_ptr, n_observers, scratch_ptr, scratch_bytes,
                                mask_ptr, status_ptr=0, occupancy_ptr=0, eye=None, max_range=0, max_blocks=0):
        """rt_terrain_visibility_field_device: the same into device arrays -- observers_ptr n_observers records of
        four int32 (pack_observers), scratch_ptr at least visibility_scratch_bytes(origin, spacing, dims) bytes,
        mask_ptr nx ny nz uint32, status_ptr 4 uint32 or 0, occupancy_ptr the caller's bit words or 0 for the
        terrain's own -- enqueued on the device's stream with no host synchronisation and no allocation.  An invalid
        observer record sees nothing.  True on success."""
        lat = lattice(origin, spacing, dims)
        opt = visibility_options(eye, max_range, max_blocks)
        self.update_shaders()
        rc = lib().rt_terrain_visibility_field_device(self.camera_compute._h, C.byref(lat), C.byref(opt),
                                                      occupancy_ptr or None, observers_ptr or None, int(n_observers),
                                                      scratch_ptr or None, int(scratch_bytes), mask_ptr or None,
                                                      status_ptr or None)
        return rc == _native.RT_OK

    def region_field(self, origin, spacing, dims, eye=None, clearance=0, occupancy=None, connectivity=26, solid=False,
                     sizes=False, max_blocks=0, status=None):
        """rt_terrain_region_field: for every point of the lattice (sample_lattice's origin, spacing and dims) the
        label of its connected region, an array shaped (nz, ny, nx) uint32: the smallest point index
        (iz * ny + iy) * nx + ix of the region, RT_REGION_NONE where the point is no member.  Members are the free
        points (with a clearance: those more than that many cells from every blocked point, as path_field's), or
        with solid=True the blocked points.  connectivity: 26 (the path field's moves) or 6 (the face moves).
        occupancy: None for the terrain's own, or bit words as sample_lattice returns them.  sizes=True:
        (labels, sizes), sizes uint32 the number of points of the point's region, 0 at a non-member.  status: a
        list that receives the four status words (completed, regions, members, the largest region's size).  None
        if the call fails.  Blocking; uses the camerarays compute."""
        lat, (nx, ny, nz) = lattice(origin, spacing, dims), (int(v) for v in dims)
        opt = region_options(eye, clearance, connectivity, solid, max_blocks)
        occ = None
        if occupancy is not None:
            occ = np.ascontiguousarray(occupancy, np.uint32)
            if occ.size != nz * ny * ((nx + 31) // 32):
                raise ValueError("region_field: occupancy must hold ceil(nx / 32) * ny * nz words")
        self.update_shaders()
        labels = np.empty((nz, ny, nx), np.uint32)
        sz = np.empty((nz, ny, nx), np.uint32) if sizes else None
        st = np.zeros(4, np.uint32)
        rc = lib().rt_terrain_region_field(self.camera_compute._h, C.byref(lat), C.byref(opt),
                                           occ.ctypes.data if occ is not None and occ.size else None, labels.ctypes.data,
                                           sz.ctypes.data if sizes and sz.size else None,
                                           st.ctypes.data if status is not None else None)
        if rc != _native.RT_OK:
            return None
        if status is not None:
            status[:] = [int(v) for v in st]
        return (labels, sz) if sizes else labels

    def region_field_device(self, origin, spacing, dims, scratch_ptr, scratch_bytes, label_ptr, size_ptr=0, status_ptr=0,
                            occupancy_ptr=0, eye=None, clearance=0, connectivity=26, solid=False, max_blocks=0):
        """rt_terrain_region_field_device: the same into device arrays -- scratch_ptr at least
        region_scratch_bytes(origin, spacing, dims, clearance) bytes, label_ptr nx ny nz uint32, size_ptr the same or
        0, status_ptr 4 uint32 or 0, occupancy_ptr the caller's bit words or 0 for the terrain's own -- a fixed
        number of launches enqueued on the device's stream with no host synchronisation and no allocation.  True on
        success."""
        lat = lattice(origin, spacing, dims)
        opt = region_options(eye, clearance, connectivity, solid, max_blocks)
        self.update_shaders()
        rc = lib().rt_terrain_region_field_device(self.camera_compute._h, C.byref(lat), C.byref(opt), occupancy_ptr or None,
                                                  scratch_ptr or None, int(scratch_bytes), label_ptr or None,
                                                  size_ptr or None, status_ptr or None)
        return rc == _native.RT_OK


def region_scratch_bytes(origin, spacing, dims, clearance=0):
    """rt_terrain_region_scratch_bytes: the bytes of region_field_device's scratch block for a lattice and a
    clearance (0 for an invalid lattice or one without points)."""
    lat = lattice(origin, spacing, dims)
    opt = region_options(clearance=clearance)
    return int(lib().rt_terrain_region_scratch_bytes(C.byref(lat), C.byref(opt)))


def region_options(eye=None, clearance=0, connectivity=26, solid=False, max_blocks=0):
    """An rt_region_options block: the eye of the terrain's own occupancy (None: the compute's Eye), the clearance in
    cells (free regions only), the connectivity (26, 6, or 0 for the default 26), the state (solid: the blocked
    points), the grids' cap."""
    opt = _native.RtRegionOptions()
    opt.size = C.sizeof(_native.RtRegionOptions)
    opt.flags = 0
    if eye is not None:
        opt.flags |= _native.RT_RAYS_EYE
        opt.eye[:] = [float(x) for x in np.asarray(eye, np.float32).reshape(3)]
    opt.max_blocks = int(max_blocks)
    opt.clearance_cells = int(clearance)
    opt.connectivity = int(connectivity)
    opt.state = 1 if solid else 0
    return opt


def visibility_scratch_bytes(origin, spacing, dims):
    """rt_terrain_visibility_scratch_bytes: the bytes of visibility_field_device's scratch block for a lattice (0 for
    an invalid lattice or one without points)."""
    lat = lattice(origin, spacing, dims)
    return int(lib().rt_terrain_visibility_scratch_bytes(C.byref(lat)))


def visibility_options(eye=None, max_range=0, max_blocks=0):
    """An rt_visibility_options block: the eye of the terrain's own occupancy (None: the compute's Eye), the range in
    cells (0: unbounded, 8190 at most), the grid's cap."""
    opt = _native.RtVisibilityOptions()
    opt.size = C.sizeof(_native.RtVisibilityOptions)
    opt.flags = 0
    if eye is not None:
        opt.flags |= _native.RT_RAYS_EYE
        opt.eye[:] = [float(x) for x in np.asarray(eye, np.float32).reshape(3)]
    opt.max_blocks = int(max_blocks)
    opt.max_range = int(max_range)
    return opt


VIS_MAX_OBSERVERS = 32
VIS_MAX_DIRECTION = 4095


def pack_observers(observers, directions, dims):
    """The observer records of a visibility field, an (n, 4) int32 array of x, y, z, kind: the point observers
    ((n, 3) ix, iy, iz; kind 0) first, then the directions ((m, 3) integers towards the light; kind 1).  Either may
    be None.  ValueError for what the C call rejects: none or more than 32 in all, a point off the lattice, a zero
    direction or a component beyond +-4095."""
    nx, ny, nz = (int(v) for v in dims)
    rows = []
    for given, kind in ((observers, _native.RT_VIS_POINT), (directions, _native.RT_VIS_DIRECTION)):
        if given is None:
            continue
        a = np.asarray(given)
        if a.size == 0:
            continue
        if a.ndim == 1 and a.size == 3:
            a = a.reshape(1, 3)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("pack_observers: observers and directions are (n, 3) arrays")
        if not np.issubdtype(a.dtype, np.integer):
            if not np.all(np.asarray(a, np.float64) == np.rint(np.asarray(a, np.float64))):
                raise ValueError("pack_observers: observers and directions are integers (see lattice_direction)")
            a = np.rint(np.asarray(a, np.float64))
        a = a.astype(np.int64)
        if kind == _native.RT_VIS_POINT:
            if (a < 0).any() or (a >= np.array([nx, ny, nz])).any():
                raise ValueError("pack_observers: a point observer is not a point of the lattice")
        else:
            if (np.abs(a) > VIS_MAX_DIRECTION).any():
                raise ValueError("pack_observers: a direction's component is beyond +-4095")
            if (a == 0).all(axis=1).any():
                raise ValueError("pack_observers: a direction is zero")
        rows.append(np.concatenate([a, np.full((a.shape[0], 1), kind, np.int64)], axis=1))
    n = sum(r.shape[0] for r in rows)
    if n < 1 or n > VIS_MAX_OBSERVERS:
        raise ValueError("pack_observers: 1..32 observers and directions in all")
    return np.ascontiguousarray(np.concatenate(rows, axis=0), np.int32)


def lattice_direction(world_dir, spacing, max_abs=255):
    """The integer direction nearest a world vector in lattice terms, for visibility_field's directions:
    round(max_abs * v / max|v|) with v_i = world_i / spacing_i, so its largest component is +-max_abs (1..4095).
    ValueError for a zero spacing or a zero vector."""
    w = np.asarray(world_dir, np.float64).reshape(3)
    s = np.asarray(spacing, np.float64).reshape(3)
    max_abs = int(max_abs)
    if not 1 <= max_abs <= VIS_MAX_DIRECTION:
        raise ValueError("lattice_direction: max_abs is 1..4095")
    if (s == 0).any() or not np.isfinite(s).all():
        raise ValueError("lattice_direction: a spacing is zero")
    v = w / s
    top = np.abs(v).max()
    if not np.isfinite(v).all() or top == 0:
        raise ValueError("lattice_direction: the vector is zero")
    return tuple(int(c) for c in np.rint(max_abs * v / top))


def path_scratch_bytes(origin, spacing, dims, clearance=0):
    """rt_terrain_path_scratch_bytes: the bytes of path_field_device's scratch block for a lattice and a clearance
    (0 for an invalid lattice or one without points)."""
    lat = lattice(origin, spacing, dims)
    opt = path_options(clearance=clearance)
    return int(lib().rt_terrain_path_scratch_bytes(C.byref(lat), C.byref(opt)))


def path_options(eye=None, clearance=0, max_cost=0, max_sweeps=0, max_blocks=0):
    """An rt_path_options block: the eye of the terrain's own occupancy (None: the compute's Eye), the clearance in
    cells, the largest cost that stays finite (0: unbounded), the sweeps (host form 0: until converged), the grids'
    cap."""
    opt = _native.RtPathOptions()
    opt.size = C.sizeof(_native.RtPathOptions)
    opt.flags = 0
    if eye is not None:
        opt.flags |= _native.RT_RAYS_EYE
        opt.eye[:] = [float(x) for x in np.asarray(eye, np.float32).reshape(3)]
    opt.max_blocks = int(max_blocks)
    opt.clearance_cells = int(clearance)
    opt.max_cost = int(max_cost)
    opt.max_sweeps = int(max_sweeps)
    return opt


def seed_indices(seeds, dims):
    """Flat uint32 point indices, (iz * ny + iy) * nx + ix, from (n, 3) ix, iy, iz rows or from flat indices."""
    nx, ny, nz = (int(v) for v in dims)
    s = np.asarray(seeds)
    if s.ndim == 2 and s.shape[1] == 3:
        s = s.astype(np.int64)
        if s.size and ((s < 0).any() or (s >= np.array([nx, ny, nz])).any()):
            raise ValueError("path_field: a seed is not a point of the lattice")
        s = (s[:, 2] * ny + s[:, 1]) * nx + s[:, 0]
    return np.ascontiguousarray(np.asarray(s).reshape(-1), np.uint32)


_PATH_WEIGHT = (0, 3, 4, 5)


def follow_flow(flow, start, max_len=None):
    """The lattice points from `start` (ix, iy, iz) along a path field's flow to a seed, both ends included: a
    (k, 3) int array of ix, iy, iz; empty from a point with no flow (RT_PATH_NONE).  Stops after max_len points
    (None: the lattice's points, which no path exceeds).  Host code."""
    flow = np.asarray(flow)
    nz, ny, nx = flow.shape
    x, y, z = (int(v) for v in start)
    limit = flow.size if max_len is None else int(max_len)
    out = []
    while len(out) < limit:
        c = int(flow[z, y, x])
        if c == _native.RT_PATH_NONE:
            return np.zeros((0, 3), np.int64) if not out else np.array(out, np.int64)
        out.append((x, y, z))
        if c == 13:
            break
        x, y, z = x + c % 3 - 1, y + c // 3 % 3 - 1, z + c // 9 - 1
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
            break
    return np.array(out, np.int64).reshape(-1, 3)


def path_cost_along(points):
    """The summed 3-4-5 weights of the moves between consecutive points of a (k, 3) lattice path."""
    p = np.asarray(points, np.int64).reshape(-1, 3)
    steps = (np.diff(p, axis=0) != 0).sum(axis=1)
    return int(sum(_PATH_WEIGHT[int(k)] for k in steps))


def distance_scratch_bytes(origin, spacing, dims):
    """rt_terrain_distance_scratch_bytes: the bytes of distance_field_device's scratch block for a lattice (0 for an
    invalid lattice or one without points)."""
    lat = lattice(origin, spacing, dims)
    return int(lib().rt_terrain_distance_scratch_bytes(C.byref(lat)))


def distance_options(eye=None, max_cells=0, max_blocks=0):
    """An rt_distance_options block: the eye of the terrain's own occupancy (None: the compute's Eye), the largest
    distance in cells that stays finite (0: unbounded), the grids' cap."""
    opt = _native.RtDistanceOptions()
    opt.size = C.sizeof(_native.RtDistanceOptions)
    opt.flags = 0
    if eye is not None:
        opt.flags |= _native.RT_RAYS_EYE
        opt.eye[:] = [float(x) for x in np.asarray(eye, np.float32).reshape(3)]
    opt.max_blocks = int(max_blocks)
    opt.max_cells = int(max_cells)
    return opt


def mesh_scratch_bytes(origin, spacing, dims):
    """rt_terrain_mesh_scratch_bytes: the bytes of extract_mesh_device's scratch block for a lattice (0 for an
    invalid lattice or one without cells)."""
    lat = lattice(origin, spacing, dims)
    return int(lib().rt_terrain_mesh_scratch_bytes(C.byref(lat)))


def field_options(eye=None, normals=False, max_blocks=0):
    """An rt_field_options block: the eye (None: the compute's Eye), RT_FIELD_NORMAL, the grid's cap."""
    opt = _native.RtFieldOptions()
    opt.size = C.sizeof(_native.RtFieldOptions)
    opt.flags = _native.RT_FIELD_NORMAL if normals else 0
    if eye is not None:
        opt.flags |= _native.RT_RAYS_EYE
        opt.eye[:] = [float(x) for x in np.asarray(eye, np.float32).reshape(3)]
    opt.max_blocks = int(max_blocks)
    return opt


def lattice(origin, spacing, dims):
    """An rt_lattice block: origin and spacing (3 floats each), dims (nx, ny, nz)."""
    lat = _native.RtLattice()
    lat.origin[:] = [float(x) for x in np.asarray(origin, np.float32).reshape(3)]
    lat.spacing[:] = [float(x) for x in np.asarray(spacing, np.float32).reshape(3)]
    lat.dims[:] = [int(x) for x in dims]
    return lat


def _xyz_rows(a):
    """(n, 3) float32, contiguous, of (n, 3) rows or of (n, 4) rows whose spare word is dropped."""
    a = np.asarray(a, np.float32)
    if a.ndim == 2 and a.shape[1] == 4:
        a = a[:, :3]
    return np.ascontiguousarray(a).reshape(-1, 3)


def point_options(eye=None, ao_samples=0, seed=0, max_blocks=0):
    """An rt_point_options block: the eye (None: the compute's Eye), the AO rays a point (0..16), the seed of
    their directions' hash, the grid's cap."""
    opt = _native.RtPointOptions()
    opt.size = C.sizeof(_native.RtPointOptions)
    opt.flags = 0
    if eye is not None:
        opt.flags |= _native.RT_RAYS_EYE
        opt.eye[:] = [float(x) for x in np.asarray(eye, np.float32).reshape(3)]
    opt.max_blocks = int(max_blocks)
    opt.ao_samples = int(ao_samples)
    opt.seed = int(seed) & 0xffffffff
    return opt


def pack_points(points):
    """The field queries' device layout: (n, 4) float32 rows x y z 0 (one 16-byte load per point)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    out = np.zeros((len(p), 4), np.float32)
    out[:, 0:3] = p
    return out


RAY_MODES = {"auto": 0, "segments": _native.RT_RAYS_FORCE_SEGMENTS, "lanes": _native.RT_RAYS_FORCE_LANES}


def ray_options(eye=None, mode="auto", max_blocks=0):
    """An rt_ray_options block: the LOD eye (None: the compute's Eye), the kernel shape, the lanes grid's cap."""
    if mode not in RAY_MODES:
        raise ValueError("ray query mode %r: one of %s" % (mode, sorted(RAY_MODES)))
    opt = _native.RtRayOptions()
    opt.size = C.sizeof(_native.RtRayOptions)
    opt.flags = RAY_MODES[mode]
    if eye is not None:
        opt.flags |= _native.RT_RAYS_EYE
        opt.eye[:] = [float(x) for x in np.asarray(eye, np.float32).reshape(3)]
    opt.max_blocks = int(max_blocks)
    return opt


def surface_options(eye=None, mode="auto", max_blocks=0, t_min=None, t_max=None, stepmod=None, max_steps=0,
                    ray_range=False):
    """An rt_surface_options block: ray_options' fields, and with any of t_min, t_max, stepmod, max_steps given
    RT_SURFACE_PARAMS with the others at their defaults (0.01, 5000, 1, unbounded)."""
    if mode not in RAY_MODES:
        raise ValueError("ray query mode %r: one of %s" % (mode, sorted(RAY_MODES)))
    opt = _native.RtSurfaceOptions()
    opt.size = C.sizeof(_native.RtSurfaceOptions)
    opt.flags = RAY_MODES[mode]
    if eye is not None:
        opt.flags |= _native.RT_RAYS_EYE
        opt.eye[:] = [float(x) for x in np.asarray(eye, np.float32).reshape(3)]
    opt.max_blocks = int(max_blocks)
    if t_min is not None or t_max is not None or stepmod is not None or max_steps:
        opt.flags |= _native.RT_SURFACE_PARAMS
        opt.t_min = 0.01 if t_min is None else float(t_min)
        opt.t_max = 5000.0 if t_max is None else float(t_max)
        opt.stepmod = 1.0 if stepmod is None else float(stepmod)
        opt.max_steps = int(max_steps)
    if ray_range:
        opt.flags |= _native.RT_SURFACE_RAY_RANGE
    return opt


def pack_rays(origins, dirs, ranges=None):
    """The device form's ray layout: (n, 8) float32 rows ox oy oz 0 dx dy dz 0 (two 16-byte loads per ray); with
    ranges (n, 2) the spare words are the ray's t_min and t_max (surface queries' RT_SURFACE_RAY_RANGE)."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("pack_rays: %d origins, %d dirs" % (len(o), len(d)))
    out = np.zeros((len(o), 8), np.float32)
    out[:, 0:3] = o
    out[:, 4:7] = d
    if ranges is not None:
        r = np.asarray(ranges, np.float32).reshape(-1, 2)
        if len(r) != len(o):
            raise ValueError("pack_rays: %d rays, %d ranges" % (len(o), len(r)))
        out[:, 3] = r[:, 0]
        out[:, 7] = r[:, 1]
    return out


def render_batch(terrains, shard_rank=0, shard_count=1):
    """rt_terrain_render_batch: Terrain.render_device for up to 24 Terrains at once (RT_MAX_BATCH) (one GPU,
    one resolution, landscape, macro set and noise).  Each frame lands in its own Device's
    framebuffer; the work is enqueued on the first terrain's device stream and the others'
    streams wait for it."""
    n = len(terrains)
    for t in terrains:
        t.update_shaders()
    cams = (C.c_void_p * n)(*[t.camera_compute._h for t in terrains])
    scrs = (C.c_void_p * n)(*[t.compute._h for t in terrains])
    check(lib().rt_terrain_render_batch(cams, scrs, n, shard_rank, shard_count), "terrain_render_batch")


def render_batch_packed(terrains, shard_rank, shard_count, dst_ptr, frame_stride):
    """rt_terrain_render_batch_packed (ABI 7): the batch's shard (frame f traces shard (rank + f) % count)
    with its pixels stored straight into the packed device buffer dst_ptr + f * frame_stride (rt_shard_pack's
    layout) instead of the framebuffers: no pack launch before the gather (RGBA8-only devices)."""
    n, cams, scrs = _batch_handles(terrains)
    check(lib().rt_terrain_render_batch_packed(cams, scrs, n, shard_rank, shard_count, dst_ptr, frame_stride),
          "terrain_render_batch_packed")


def _batch_handles(terrains):
    n = len(terrains)
    for t in terrains:
        t.update_shaders()
    return n, (C.c_void_p * n)(*[t.camera_compute._h for t in terrains]), (C.c_void_p * n)(*[t.compute._h for t in terrains])


def prepass_batch(terrains, first, count, camera_out_ptr):
    """rt_terrain_prepass_batch: the prepass of frames [first, first + count) of the batch, frame
    f's CameraResults to camera_out_ptr + f * 16 KiB (device memory)."""
    n, cams, scrs = _batch_handles(terrains)
    check(lib().rt_terrain_prepass_batch(cams, scrs, n, first, count, camera_out_ptr), "terrain_prepass_batch")


def trace_batch(terrains, shard_rank, shard_count, camera_in_ptr):
    """rt_terrain_trace_batch: setTargetDepths + tracescreen of the batch from gathered
    CameraResults (frame f at camera_in_ptr + f * 16 KiB)."""
    n, cams, scrs = _batch_handles(terrains)
    check(lib().rt_terrain_trace_batch(cams, scrs, n, shard_rank, shard_count, camera_in_ptr), "terrain_trace_batch")


def prepass_ahead(terrains):
    """rt_terrain_prepass_ahead (ABI 5): queue the batch's prepass on the GPU's side stream, after
    the last setTargetDepths of the batches the first terrain's device leads.  Issue it before
    the previous batch's trace_ahead / render_batch; trace_ahead(terrains) consumes it."""
    n, cams, scrs = _batch_handles(terrains)
    check(lib().rt_terrain_prepass_ahead(cams, scrs, n), "terrain_prepass_ahead")


def trace_ahead(terrains, shard_rank=0, shard_count=1):
    """rt_terrain_trace_ahead (ABI 5): setTargetDepths + tracescreen after the batch's ahead
    prepass (the full render_batch when none covers these frames or a camera changed since)."""
    n, cams, scrs = _batch_handles(terrains)
    check(lib().rt_terrain_trace_ahead(cams, scrs, n, shard_rank, shard_count), "terrain_trace_ahead")


def _cbuffer_matrix(m):
    """Bytes of XMMatrixTranspose(M) -- what the engine writes for a float4x4 cbuffer variable."""
    return np.ascontiguousarray(np.asarray(m, np.float32).T)


def shard_bytes(device, rank, count):
    return int(lib().rt_shard_bytes(device._h, rank, count))


def shard_pack(device, rank, count, dst_ptr):
    check(lib().rt_shard_pack(device._h, rank, count, dst_ptr), "shard_pack")


def shard_unpack(device, rank, count, src_ptr):
    check(lib().rt_shard_unpack(device._h, rank, count, src_ptr), "shard_unpack")


def _shard_batch(fn, what, devices, shards, count, ptrs):
    n = len(devices)
    if not (n == len(shards) == len(ptrs)):
        raise ValueError(f"{what}: devices, shards and buffers differ in length")
    if n == 0:
        return
    hs = (C.c_void_p * n)(*[d._h for d in devices])
    ss = (C.c_int * n)(*[int(s) for s in shards])
    ps = (C.c_void_p * n)(*[int(p) for p in ptrs])
    check(fn(hs, ss, count, ps, n), what)


def shard_pack_batch(devices, shards, count, dst_ptrs):
    """rt_shard_pack_batch: device i's shard shards[i] -> dst_ptrs[i], one launch on devices[0]'s stream."""
    _shard_batch(lib().rt_shard_pack_batch, "shard_pack_batch", devices, shards, count, dst_ptrs)


def shard_unpack_batch(devices, shards, count, src_ptrs):
    """rt_shard_unpack_batch: src_ptrs[i] -> device i's shard shards[i], one launch on devices[0]'s stream."""
    _shard_batch(lib().rt_shard_unpack_batch, "shard_unpack_batch", devices, shards, count, src_ptrs)


class FrameRing:
    """Frames in flight: `depth` complete frame contexts (Device + Terrain: own constants,
    CameraResults/CellDistance, ray buffers and framebuffer), each on its own non-blocking HIP
    stream, with frames dealt round-robin.  This is the D3D swap chain's queued frames
    (IDevice::present with a frame-latency queue, DeviceDirect3D.cpp:234-257) made explicit:
    frame i+1's camerarays prepass and primary phase run on the CUs that frame i's ray tail
    leaves idle, instead of waiting for it.  Every frame is still computed in full and
    independently; a slot is reused only after its previous frame (i - depth) has completed on
    that slot's stream.  depth=1 is the reference's one-frame-at-a-time behaviour.
    graph=True: each slot replays its frame as captured hipGraphs (RT_DEVICE_GRAPH).
    batch=B: a slot is B frames rendered by one rt_terrain_render_batch (B devices, the
    batch on the first one's stream); render_batch() queues the next B frames.
    lookahead=True (not with graph): render_batch(ahead=True) also queues the NEXT group's prepass
    on the GPU's side stream before this batch's trace (rt_terrain_prepass_ahead), so it runs
    beside this trace instead of in front of the next one; set the next frames' cameras before
    that call (a camera written after it makes the next batch prepass again, in line)."""

    def __init__(self, width, height, depth=3, gpu=0, theme="nomadplains", camera=None, time_of_day=0.3,
                 graph=False, batch=1, float_output=False, lookahead=False, gated=False, **terrain_kw):
        self.depth, self.frame, self.batch = int(depth), 0, int(batch)
        if lookahead and graph:
            raise ValueError("lookahead runs the prepass on a side stream: not with graph=True")
        self.lookahead, self._ahead = bool(lookahead), set()  # groups with an ahead prepass queued
        # one HIP hardware queue per busy stream: the groups', the side stream, torch's default
        # (DESIGN.md section 7); fewer make two groups share one and their batches serialise
        want = self.depth + 1 + int(self.lookahead)
        try:
            have = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
        except ValueError:
            have = 4
        if self.depth > 1 and have < want:
            warnings.warn(f"FrameRing: {want} busy streams but GPU_MAX_HW_QUEUES={have}; set it to >= {want} "
                          "before HIP starts, or the batches in flight may run one after the other", stacklevel=2)
        self.slots = []
        for _ in range(self.depth * self.batch):
            dev = DeviceFactory.construct(DeviceAPI.HIP, width, height, gpu=gpu, graph=graph,
                                          float_output=float_output, gated=gated)
            if dev is None:
                raise RuntimeError("device create failed: " + lib().rt_last_error().decode())
            ter = Terrain(dev, theme, **terrain_kw)
            ter.create()
            if not ter.reload():
                raise RuntimeError("shader load failed: " + lib().rt_last_error().decode())
            if camera is not None:
                ter.set_camera(camera)
            ter.set_time_of_day(time_of_day)
            ter.update_shaders()
            if len(self.slots) % self.batch:  # a batch's devices share the first one's stream
                dev.set_stream(self.slots[len(self.slots) - len(self.slots) % self.batch][0].stream())
            self.slots.append((dev, ter))

    def next_slot(self):
        return self.slots[self.frame % self.depth]

    def group(self, frames=None):
        """The next slot group (its first `frames` slots, default all `batch`)."""
        g = (self.frame // self.batch) % self.depth
        n = self.batch if frames is None else int(frames)
        if not 1 <= n <= self.batch:
            raise ValueError("frames must be 1..batch")
        return self.slots[g * self.batch:g * self.batch + n]

    def render_batch(self, shard_rank=0, shard_count=1, present=True, frames=None, ahead=True):
        """Queue the next `batch` frames (or the first `frames` of them: a partial batch) as one
        batch on the next slot group; returns their Devices in frame order (each complete once
        its stream reaches this point).  With lookahead, ahead=False skips queueing the next
        group's prepass (the last batch of a run)."""
        group = self.group(frames)
        terrains = [t for _, t in group]
        if not self.lookahead:
            render_batch(terrains, shard_rank, shard_count)
        else:
            g = (self.frame // self.batch) % self.depth
            if g not in self._ahead:
                prepass_ahead(terrains)
            self._ahead.discard(g)
            nxt = (g + 1) % self.depth
            if ahead and nxt != g:
                prepass_ahead([t for _, t in self.slots[nxt * self.batch:(nxt + 1) * self.batch]])
                self._ahead.add(nxt)
            trace_ahead(terrains, shard_rank, shard_count)
        devs = [d for d, _ in group]
        if present:
            for d in devs:
                d.present()
        self.frame += self.batch
        return devs

    def render(self, shard_rank=0, shard_count=1, camera=None, present=True):
        """Queue one frame on the next slot; returns its Device (the frame is complete once
        that device's stream reaches this point: Device.synchronize / readback)."""
        dev, ter = self.next_slot()
        if camera is not None:
            ter.set_camera(camera)
            ter.update_terrain()
        ter.render_device(shard_rank, shard_count)
        if present:
            dev.present()
        self.frame += 1
        return dev

    def synchronize(self):
        for dev, _ in self.slots:
            dev.synchronize()

    def set_profiling(self, on):
        for dev, _ in self.slots:
            check(lib().rt_device_set_profiling(dev._h, 1 if on else 0), "set_profiling")

    def kernel_time(self):
        """(total ms, launches) of tracescreen launches recorded since the last call, all slots."""
        tot, n = 0.0, 0
        for dev, _ in self.slots:
            kms, kn = C.c_double(), C.c_int()
            check(lib().rt_device_kernel_time(dev._h, C.byref(kms), C.byref(kn)), "kernel_time")
            tot, n = tot + kms.value, n + kn.value
        return tot, n

    def destroy(self):
        # any order is safe: a group's devices borrow its first device's stream, and the runtime
        # keeps a lent stream alive until its last user is destroyed (rt_stream_refs)
        for dev, _ in reversed(self.slots):
            dev.destroy()
        self.slots = []
