// hip_adapter.h -- the reference engine's device interfaces implemented over the
// frosttrace C-ABI (include/frosttrace.h).  Drop-in for Adapters/DeviceDirect3D +
// ComputeDirect3D + ShaderVariableDirect3D + TextureDirect3D: Terrain, Raytracer and
// Flyby keep calling IDevice / ICompute / IShaderVariable / IShaderArray / ITexture.
//
// Compiled against the reference headers (-I gpuraytrace); see INTEGRATION.md.
#pragma once

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "Factories/ICompute.h"
#include "Factories/IDevice.h"
#include "Factories/IRecorder.h"
#include "Factories/ITexture.h"
#include "frosttrace.h"

// DeviceAPI::HIP once Factories/IDevice.h gains it.
const DeviceAPI::T kDeviceApiHip = static_cast<DeviceAPI::T>(3);

// ShaderVariableDirect3D.cpp:59-90 / 195-202: write copies the reflected size into a
// shadow uploaded lazily on the next run.
class ShaderVariableHIP : public IShaderVariable
{
public:
    ShaderVariableHIP(const std::string& name, rt_variable v) : IShaderVariable(name, nullptr), v(v)
    { setWritable(true); }
    void write(void* data) override { rt_variable_write(v, data); }

private:
    rt_variable v;
};

// UAVBufferD3D (ShaderVariableDirect3D.cpp:92-193) and StructuredBufferD3D (:204-281).
class ShaderArrayHIP : public IShaderArray
{
public:
    ShaderArrayHIP(const std::string& name, rt_array a) : IShaderArray(name), a(a) { setWritable(true); }
    bool create(unsigned int elements) override { return rt_array_create(a, elements) == RT_OK; }
    void* map() override { return rt_array_map(a); }
    void unmap() override { rt_array_unmap(a); }
    void write(void* data) override { rt_array_write(a, data); }

private:
    rt_array a;
};

// TextureDirect3D.cpp:40-164
class TextureHIP : public ITexture
{
public:
    explicit TextureHIP(rt_device dev);
    ~TextureHIP() override;
    bool create(const std::string& path) override;
    bool create(TextureDimensions::T dimensions, TextureFormat::T format, int width, int height, const void* data,
                TextureBinding::T binding, CPUAccess::T cpuFlags) override;
    rt_texture handle() const { return tex; }

private:
    rt_texture tex = nullptr;
};

// ComputeDirect3D.cpp:403-614
class ComputeHIP : public ICompute
{
public:
    explicit ComputeHIP(rt_device dev);
    ~ComputeHIP() override;
    bool create(const std::string& directory, const std::string& fileName, const std::string& main,
                const ThreadSize& ts, const std::vector<MacroType>& macros) override;
    void run(unsigned int dispatchX, unsigned int dispatchY, unsigned int dispatchZ) override;
    IShaderVariable* getVariable(const std::string& name) override;
    IShaderArray* getArray(const std::string& name) override;
    IShaderBuffer* getBuffer(const std::string& name) override;
    bool swap() override;
    void setTexture(int stage, ITexture* texture) override;
    // (adapter extension) rt_terrain_trace_rays (ABI 9, additive): what n rays of the host's own hit, marched as
    // camerarays.hlsl:12-21 marches its pixel rays with this compute's landscape, tables and constants.  origins,
    // dirs: 3n floats (dirs as given: their length enters the first step); results: 4n floats (the last sample's
    // position, the hit distance or 5000 for a miss); eye: the level-of-detail eye (3 floats), nullptr = the
    // compute's Eye variable.  Blocking.  The reference's only hit query is the last prepass (Flyby.cpp:44-90).
    bool traceRays(const float* origins, const float* dirs, int n, float* results, const float* eye = nullptr);
    // (adapter extension) rt_terrain_trace_surface (ABI 9, additive): where those rays meet the SURFACE and its
    // normal there -- the refined march of tracescreen's pixels (tracing.hlsl:47-105, skiprefine off) and getNormal
    // (:107-116): picking and placement.  results: 8n floats (the last sample's position, its distance | the unit
    // normal, the density: a hit is density > 0, a miss has a zero normal); ranges: 2n floats t_min_i, t_max_i,
    // nullptr = 0.01 to 5000; eye: the LOD eye and getNormal's, nullptr = the compute's Eye variable.  Blocking.
    bool traceSurface(const float* origins, const float* dirs, int n, float* results, const float* eye = nullptr,
                      const float* ranges = nullptr);
    rt_compute handle() const { return cs; }

private:
    rt_compute cs = nullptr;
    ThreadSize pending{};
    std::map<std::string, std::unique_ptr<ShaderVariableHIP>> variables;
    std::map<std::string, std::unique_ptr<ShaderArrayHIP>> arrays;
};

// DeviceDirect3D.cpp:77-267.  present() ends the frame; the linear RGBA8 framebuffer
// stays in HBM and readback() copies it out (recorder / window blit).
class DeviceHIP : public IDevice
{
public:
    explicit DeviceHIP(IWindow* window);
    ~DeviceHIP() override;
    bool create() override;
    void present() override;
    void flush() override;
    ICompute* createCompute() override;
    ITexture* createTexture() override;
    bool readback(void* dst, size_t rowPitch) const;
    // (adapter extension) the frame without a host synchronisation per frame, over rt_readback_* (ABI 9, additive):
    // readbackSubmit captures the frame readback() would return now and hands out its ticket (an RGBA8 ring of 3
    // captures, made at the first submit); readbackWait returns its tight RGBA8 rows, valid until readbackRelease.
    // The reference's present() maps its staging texture every frame (DeviceDirect3D.cpp:244-256).
    bool readbackSubmit(unsigned long long* ticket);
    const void* readbackWait(unsigned long long ticket);
    bool readbackRelease(unsigned long long ticket);
    rt_device handle() const { return dev; }
    void setRecorder(class RecorderHIP* r) { recorder = r; } // DeviceDirect3D::setRecorder (:229-232)
    // (adapter extension, before create) rt_device_create's flags, e.g. RT_DEVICE_DEFERRED (ABI 9): the reference's
    // IDevice::create takes none
    void setFlags(unsigned f) { flags = f; }

private:
    rt_device dev = nullptr;
    rt_readback ring = nullptr;
    unsigned flags = 0;
    class RecorderHIP* recorder = nullptr;
};

// RecorderWinAPI (Adapters/RecorderWinAPI.cpp) over rt_recorder_*: RecorderFactory::construct
// makes one for a DeviceHIP; it attaches to the device, whose present() then writes every
// frame while recording (DeviceDirect3D.cpp:242-256), swizzled to RGB32 on the GPU.  The sink
// is a raw-video file (+ time-stamp index) instead of Media Foundation's output.wmv.
class RecorderHIP : public IRecorder
{
public:
    RecorderHIP(IDevice* device, int frameRate, bool fixedSpeed) : device(device), frameRate(frameRate),
        fixedSpeed(fixedSpeed) { }
    ~RecorderHIP() override;
    bool create() override;
    void start() override { IRecorder::start(); rt_recorder_start(rec); }
    void stop() override { IRecorder::stop(); rt_recorder_stop(rec); }
    void write(void* frame, int stride) override { rt_recorder_write(rec, frame, stride); }
    // (adapter extension, after create) rt_recorder_set_async: depth 1..8 = present() submits the frame to a ring and
    // writes the older frames that are ready instead of waiting for the frame; 0 = synchronous.  Same files.
    bool setAsync(int depth) { return rt_recorder_set_async(rec, depth) == RT_OK; }
    rt_recorder handle() const { return rec; }

private:
    IDevice* device;
    int frameRate;
    bool fixedSpeed;
    rt_recorder rec = nullptr;
};
