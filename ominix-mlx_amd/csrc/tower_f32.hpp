// What the two float32 towers of DeepSeek-OCR-2 (sam_encoder.hip, vcf_encoder.hip) share on the host side: the weight store by checkpoint
// key, scratch that grows per role and is counted, and the float32 GEMM call with its epilogues.
#pragma once
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "gemm.hpp"

namespace omx {
namespace tower {

inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 8192); }

struct Store {
    std::map<std::string, float*> w;              // device float32 tensors by key
    std::map<std::string, std::vector<int64_t>> shape;
    std::string prefix;                           // the checkpoint prefix, for the error texts only
    ~Store() { for (auto& kv : w) (void)hipFree(kv.second); }
    int load(const char* who, const char* name, const float* host, const int64_t* shp, int ndim) {
        OMX_REQUIRE(name && host && shp && ndim >= 1 && ndim <= 4, "%s: bad argument", who);
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) { OMX_REQUIRE(shp[i] >= 1, "%s: %s: empty dimension", who, name); n *= (size_t)shp[i]; }
        const std::string key(name);
        auto it = w.find(key);
        if (it != w.end()) { (void)hipDeviceSynchronize(); (void)hipFree(it->second); w.erase(it); }
        float* dev = nullptr;
        OMX_HIP_CHECK(hipMalloc((void**)&dev, n * sizeof(float)));
        if (hipMemcpy(dev, host, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dev); return omx::set_error("%s: %s: copy to the device failed", who, name); }
        w[key] = dev;
        shape[key] = std::vector<int64_t>(shp, shp + ndim);
        return 0;
    }
    size_t count(const std::string& key) const {
        auto it = shape.find(key);
        if (it == shape.end()) return 0;
        size_t n = 1;
        for (int64_t d : it->second) n *= (size_t)d;
        return n;
    }
    int64_t dim(const std::string& key, int axis) const {
        auto it = shape.find(key);
        return it == shape.end() || axis >= (int)it->second.size() ? 0 : it->second[axis];
    }
    // a tensor by key: required (WeightNotFound) or optional (null); its element count is checked where it is present.  The first
    // missing or misshapen tensor is the one reported.
    const float* find(const std::string& key, size_t want, bool required, int* err) const {
        if (*err) return nullptr;
        auto it = w.find(key);
        if (it == w.end()) {
            if (required) *err = omx::set_error("WeightNotFound: %s%s", prefix.c_str(), key.c_str());
            return nullptr;
        }
        if (count(key) != want) {
            *err = omx::set_error("ShapeMismatch: %s%s has %zu elements, the config expects %zu", prefix.c_str(), key.c_str(), count(key), want);
            return nullptr;
        }
        return it->second;
    }
};

template <int ROLES>
struct Scratch {
    float* buf[ROLES] = {};
    size_t cap[ROLES] = {};
    ~Scratch() { for (float* p : buf) if (p) (void)hipFree(p); }
    int reserve(int role, size_t elems, hipStream_t s) {
        if (elems <= cap[role]) return 0;
        OMX_HIP_CHECK(hipStreamSynchronize(s));
        if (buf[role]) OMX_HIP_CHECK(hipFree(buf[role]));
        buf[role] = nullptr; cap[role] = 0;
        OMX_HIP_CHECK(hipMalloc((void**)&buf[role], elems * sizeof(float)));
        cap[role] = elems;
        return 0;
    }
    size_t bytes() const {
        size_t n = 0;
        for (size_t c : cap) n += c;
        return n * sizeof(float);
    }
};

// out [M, N] (rows ldc apart) = resid + act(a [M, K] . w [N, K]^T + bias); act 0 none, 1 the exact GELU, 2 the tanh GELU
struct Linear {
    const float* a; const float* w; const float* bias; const float* resid; float* out;
    int M, N, K; int64_t ldc, ldr; int gelu;
};
inline int gemm(const Linear& l, hipStream_t s) {
    GemmF32 g = {};
    g.a = l.a; g.b = l.w; g.bias = l.bias; g.resid = l.resid; g.out = l.out;
    g.M = l.M; g.N = l.N; g.K = l.K; g.lda = l.K; g.ldb = l.K; g.ldc = l.ldc ? l.ldc : l.N; g.ldr = l.ldr ? l.ldr : l.N;
    g.batch = 1; g.alpha = 1.0f;
    g.gelu = l.gelu;
    return launch_gemm_f32(g, s);
}

}  // namespace tower
}  // namespace omx
