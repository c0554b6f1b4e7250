// sva.hpp -- C++ host mirror of the reference's interface for the stereo hot
// path, layered on the C-ABI in sva.h.  Header-only; no OpenCV, no torch.
//
// It keeps the reference's names, argument meaning and error behaviour so a
// call site in CameraStereoVision.cpp reads the same:
//   Camera               include/Camera.h:6-21, src/Camera.cpp:6-34
//   pairType             include/functions.h:8-19
//   getCameraPairs       src/functions.cpp:148-213 (incl. the :205 quirk, opt-out)
//   getGroups            src/functions.cpp:107-116
//   bresenham            src/functions.cpp:253-321
//   getAbsDiff           src/functions.cpp:215-218 (on raw 8-bit views)
//   computeDisparity     NEW: replaces the inline hot loop
//                        src/CameraStereoVision.cpp:44-95 with one GPU call
//   disparityToDepth     src/CameraStereoVision.cpp:47,98-100
//   getIdealRef / saveImage / loadImage / calculateAverageError
//                        src/functions.cpp:323-354 (OpenCV-YAML matrix files),
//   refError             src/CameraStereoVision.cpp:107-110,118-119
// Host-side helpers (Camera math, bresenham, pair tables) run on the CPU as in
// the reference -- they are per-call scalars, not the hot path.  Everything
// per-pixel runs on the GPU through sva.h.  Errors are reported as
// sva::Error exceptions on the C++ side (the reference throws cv::Exception on
// bad input); nothing throws across the C-ABI itself.
#pragma once

#include <algorithm>
#include <array>
#include <filesystem>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "sva.h"

namespace sva {

struct Point2i {
    int x = 0, y = 0;
    Point2i() = default;
    Point2i(int x_, int y_) : x(x_), y(y_) {}
    Point2i operator+(const Point2i& o) const { return {x + o.x, y + o.y}; }
    Point2i operator-(const Point2i& o) const { return {x - o.x, y - o.y}; }
    bool operator==(const Point2i& o) const { return x == o.x && y == o.y; }
};

struct Point3d {
    double x = 0, y = 0, z = 0;
    Point3d() = default;
    Point3d(double x_, double y_, double z_) : x(x_), y(y_), z(z_) {}
    Point3d operator+(const Point3d& o) const { return {x + o.x, y + o.y, z + o.z}; }
    Point3d operator-(const Point3d& o) const { return {x - o.x, y - o.y, z - o.z}; }
    Point3d operator*(double s) const { return {x * s, y * s, z * s}; }
    Point3d operator/(double s) const { return {x / s, y / s, z / s}; }
};

inline double norm(const Point3d& p) { return std::sqrt(p.x * p.x + p.y * p.y + p.z * p.z); }
inline double norm(const Point2i& p) {
    return std::sqrt((double)p.x * p.x + (double)p.y * p.y);
}

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string& m) : std::runtime_error(m), status(s) {}
};

// class Camera -- include/Camera.h:6-21 (public fields, same constructor).
class Camera {
public:
    Camera(double focal_length, Point3d position, double pixel_size_)
        : pos3D(position), f(focal_length), pixel_size(pixel_size_) {}

    Point3d pos3D;
    double f;
    double pixel_size;

    // Camera::project (src/Camera.cpp:15-21): truncation toward zero.
    Point2i project(Point3d P) const {
        double mult = f / (P.z - pos3D.z) / pixel_size;
        return {int((P.x - pos3D.x) * mult), int((P.y - pos3D.y) * mult)};
    }
    // Camera::inv_project (src/Camera.cpp:25-33).
    Point3d inv_project(Point2i px) const {
        Point3d v{px.x * pixel_size, px.y * pixel_size, f};
        return v / norm(v);
    }
    sva_camera abi() const {
        sva_camera c;
        c.f = f;
        c.pos[0] = pos3D.x;
        c.pos[1] = pos3D.y;
        c.pos[2] = pos3D.z;
        c.pixel_size = pixel_size;
        return c;
    }
};

// include/functions.h:8-19
enum pairType {
    ORTHOGONAL,
    DIAGONAL,
    TO_CENTER,
    LINE_HORIZONTAL,
    LINE_VERTICAL,
    CROSS,
    JUMP_CROSS,
    TO_CENTER_SMALL,
    MID_LEFT,
    MID_TOP
};

// getCameraPairs(cameras, pairType) -- src/functions.cpp:148-197.
inline std::vector<std::array<int, 2>> getCameraPairs(const std::vector<Camera>& cameras,
                                                      const pairType pair) {
    std::vector<std::array<int, 2>> pairs;
    const int n = (int)cameras.size();
    switch (pair) {
        case TO_CENTER:
            for (int i = 0; i < n; i++)
                if (i != 12) pairs.push_back({12, i});
            break;
        case TO_CENTER_SMALL:
            for (int o : {6, 7, 8, 11, 13, 16, 17, 18}) pairs.push_back({12, o});
            break;
        case MID_LEFT: pairs.push_back({12, 11}); break;
        case MID_TOP: pairs.push_back({12, 7}); break;
        case LINE_HORIZONTAL:
            for (int i = 10; i < 15; i++)
                if (i != 12) pairs.push_back({12, i});
            break;
        case LINE_VERTICAL:
            for (int i = 2; i < 25; i += 5)
                if (i != 12) pairs.push_back({12, i});
            break;
        case CROSS:
            for (int o : {11, 13, 7, 17}) pairs.push_back({12, o});
            break;
        case JUMP_CROSS:
            for (int o : {10, 14, 2, 24}) pairs.push_back({12, o});
            break;
        default: break;  // ORTHOGONAL, DIAGONAL: empty in the reference too
    }
    return pairs;
}

// getCameraPairs(cameras, CROSS, cameraNum) -- src/functions.cpp:199-213.
// reference_quirks = true reproduces the reference exactly: the second entry
// is {cameraNum, +5} (the literal camera 5, :205) and the upward neighbour is
// only added for cameraNum - 5 > 0 (:202).  false gives the evident intent.
inline std::vector<std::array<int, 2>> getCameraPairs(const std::vector<Camera>& cameras,
                                                      const pairType pair, int cameraNum,
                                                      bool reference_quirks = true) {
    (void)cameras;
    std::vector<std::array<int, 2>> pairs;
    if (pair != CROSS) return pairs;
    if (reference_quirks ? (cameraNum - 5 > 0) : (cameraNum - 5 >= 0))
        pairs.push_back({cameraNum, cameraNum - 5});
    if (cameraNum + 5 < 25) pairs.push_back({cameraNum, reference_quirks ? 5 : cameraNum + 5});
    if (cameraNum % 5 > 0) pairs.push_back({cameraNum, cameraNum - 1});
    if (cameraNum % 5 < 4) pairs.push_back({cameraNum, cameraNum + 1});
    return pairs;
}

// getGroups -- src/functions.cpp:107-116 ("CHESS": CROSS groups of 0,2,..,24).
inline std::vector<std::vector<std::array<int, 2>>> getGroups(std::vector<Camera>& cameras,
                                                              const std::string& groupType,
                                                              bool reference_quirks = true) {
    std::vector<std::vector<std::array<int, 2>>> groups;
    if (groupType == "CHESS")
        for (int i = 0; i < 25; i += 2)
            groups.push_back(getCameraPairs(cameras, CROSS, i, reference_quirks));
    return groups;
}

// bresenham(point2, point1) -- src/functions.cpp:253-321 (first parameter is
// the caller's pixel1).  Emits from the lower x (|dy| < |dx|) or lower y.
inline std::vector<Point2i> bresenham(Point2i point2, Point2i point1) {
    std::vector<Point2i> pts;
    auto low = [&](int x0, int y0, int x1, int y1) {
        int dx = x1 - x0, dy = y1 - y0, yi = 1;
        if (dy < 0) { yi = -1; dy = -dy; }
        int D = 2 * dy - dx, y = y0;
        for (int x = x0; x <= x1; x++) {
            pts.push_back({x, y});
            if (D > 0) { y += yi; D -= 2 * dx; }
            D += 2 * dy;
        }
    };
    auto high = [&](int x0, int y0, int x1, int y1) {
        int dx = x1 - x0, dy = y1 - y0, xi = 1;
        if (dx < 0) { xi = -1; dx = -dx; }
        int D = 2 * dx - dy, x = x0;
        for (int y = y0; y <= y1; y++) {
            pts.push_back({x, y});
            if (D > 0) { x += xi; D -= 2 * dy; }
            D += 2 * dx;
        }
    };
    if (std::abs(point2.y - point1.y) < std::abs(point2.x - point1.x)) {
        if (point1.x > point2.x) low(point2.x, point2.y, point1.x, point1.y);
        else low(point1.x, point1.y, point2.x, point2.y);
    } else {
        if (point1.y > point2.y) high(point2.x, point2.y, point1.x, point1.y);
        else high(point1.x, point1.y, point2.x, point2.y);
    }
    return pts;
}

// Non-owning 8-bit image view (the part of cv::Mat the path uses).
struct ImageView {
    const uint8_t* data = nullptr;
    int width = 0, height = 0;
    size_t pitch = 0;  // bytes per row
    ImageView() = default;
    ImageView(const uint8_t* d, int w, int h, size_t p = 0)
        : data(d), width(w), height(h), pitch(p ? p : (size_t)w) {}
    ImageView roi(int x, int y, int w, int h) const {
        if (x < 0 || y < 0 || x + w > width || y + h > height)
            throw Error(SVA_ERR_INVALID_ARG, "roi outside image");  // cv::Mat throws here too
        return ImageView(data + (size_t)y * pitch + x, w, h, pitch);
    }
};

// getAbsDiff -- src/functions.cpp:215-218: sum |m1 - m2| as double.
// Compatibility helper for call sites outside the hot path (e.g. one-off
// checks); computeDisparity never calls it -- its SADs run on the GPU.
inline double getAbsDiff(const ImageView& m1, const ImageView& m2) {
    if (m1.width != m2.width || m1.height != m2.height)
        throw Error(SVA_ERR_INVALID_ARG, "getAbsDiff: size mismatch");
    int64_t s = 0;
    for (int v = 0; v < m1.height; v++)
        for (int u = 0; u < m1.width; u++) {
            int d = (int)m1.data[v * m1.pitch + u] - (int)m2.data[v * m2.pitch + u];
            s += d < 0 ? -d : d;
        }
    return (double)s;
}

// RAII owner of one sva context (one device, one stream).
class Engine {
public:
    explicit Engine(int device = 0) {
        int s = sva_create(device, &ctx_);
        if (s != SVA_OK) throw Error(s, std::string("sva_create: ") + sva_status_string(s));
    }
    ~Engine() {
        if (ctx_) sva_destroy(ctx_);
    }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
    void* handle() const { return ctx_; }
    void check(int s) const {
        if (s != SVA_OK) throw Error(s, sva_last_error(ctx_));
    }
    // SVA_PATH_KERNEL_AUTO (default) or _COST_VOLUME, the same route (sva.h)
    void setPathKernel(int kernel) { check(sva_set_path_kernel(ctx_, kernel)); }

private:
    void* ctx_ = nullptr;
};

// Result of computeDisparity: the reference's CV_8UC1 map (values wrap mod
// 256, CameraStereoVision.cpp:89), the unwrapped map and a validity mask
// (the reference leaves skipped pixels uninitialised, :46).
struct DisparityMaps {
    int width = 0, height = 0;
    std::vector<uint8_t> disp_u8;
    std::vector<uint16_t> disp_u16;
    std::vector<uint8_t> valid;
};

// Replaces CameraStereoVision.cpp:44-95 (pairs loop incl. last-pair-wins).
// mask may be empty (width 0): every pixel selected.
inline DisparityMaps computeDisparity(Engine& eng, const std::vector<ImageView>& images,
                                      const std::vector<Camera>& cameras,
                                      const std::vector<std::array<int, 2>>& pairs,
                                      const ImageView& mask, int kernelSize,
                                      double t_near = 0.5, double t_far = 1.0) {
    if (pairs.empty()) throw Error(SVA_ERR_INVALID_ARG, "no camera pairs");
    const ImageView& first = images.at(pairs[0][0]);
    DisparityMaps out;
    out.width = first.width;
    out.height = first.height;
    const size_t n = (size_t)first.width * first.height;
    out.disp_u8.assign(n, 0);
    out.disp_u16.assign(n, 0);
    out.valid.assign(n, 0);
    std::vector<uint8_t> mask_dense;
    const uint8_t* mptr = nullptr;
    if (mask.data && mask.width) {
        if (mask.width != first.width || mask.height != first.height)
            throw Error(SVA_ERR_INVALID_ARG, "mask size mismatch");
        mask_dense.resize(n);
        for (int y = 0; y < mask.height; y++)
            for (int x = 0; x < mask.width; x++)
                mask_dense[(size_t)y * mask.width + x] = mask.data[(size_t)y * mask.pitch + x];
        mptr = mask_dense.data();
    }
    for (const auto& pr : pairs) {
        const ImageView& a = images.at(pr[0]);
        const ImageView& b = images.at(pr[1]);
        if (a.width != b.width || a.height != b.height || a.pitch != b.pitch)
            throw Error(SVA_ERR_INVALID_ARG, "pair images differ in size");
        const sva_camera ca = cameras.at(pr[0]).abi(), cb = cameras.at(pr[1]).abi();
        eng.check(sva_disparity_ref(eng.handle(), a.data, b.data, a.width, a.height, a.pitch, mptr,
                                    &ca, &cb, kernelSize, t_near, t_far, out.disp_u8.data(),
                                    out.disp_u16.data(), out.valid.data()));
    }
    return out;
}

// Mode S matcher on one rectified pair (north_star SGM).
inline std::vector<uint16_t> computeDisparitySGM(Engine& eng, const ImageView& left,
                                                 const ImageView& right,
                                                 const sva_sgm_params& p,
                                                 std::vector<float>* subpix = nullptr) {
    if (left.width != right.width || left.height != right.height || left.pitch != right.pitch)
        throw Error(SVA_ERR_INVALID_ARG, "pair images differ in size");
    std::vector<uint16_t> disp((size_t)left.width * left.height);
    float* sp = nullptr;
    if (subpix && p.subpixel) {
        subpix->resize(disp.size());
        sp = subpix->data();
    }
    eng.check(sva_disparity_sgm(eng.handle(), left.data, right.data, left.width, left.height,
                                left.pitch, &p, disp.data(), sp));
    return disp;
}

// CameraStereoVision.cpp:47,98-100 on the GPU (per-pixel f64; reference:
// multiply(disparity, pixelSize, .., CV_64F) then camDistance * f /
// pixSizeDisp, 0 where the divisor is 0).
inline std::vector<double> disparityToDepth(Engine& eng, const std::vector<uint8_t>& disparity,
                                            const Camera& c0, const Camera& c1) {
    const double camDistance = norm(c0.pos3D - c1.pos3D);
    std::vector<double> depth(disparity.size());
    eng.check(sva_disparity_to_depth(eng.handle(), disparity.data(), (int)disparity.size(),
                                     camDistance, c0.f, c0.pixel_size, depth.data()));
    return depth;
}

// ---- camera-array pairs ----------

// Match step of the pair (ref, other) on a planar array with grid pitch
// `pitch` (0.05 m in the reference, CameraStereoVision.cpp:34-39).  Camera
// `other` sits at grid offset g = round((other.pos3D - ref.pos3D) / pitch);
// Camera::project (Camera.cpp:15-21) maps a scene point at pixel q of `ref` to
// q - g * delta in `other`, so the step is -g reduced by the gcd of its
// components.  k = |major component of g|: the disparity along the major axis
// is k * delta and the baseline that converts it to depth is k * pitch.
struct PairStep {
    int dir = 0, dir_y = 0, k = 0;
    double baseline = 0.0;
};

inline PairStep pairStep(const Camera& ref, const Camera& other, double pitch = 0.05) {
    const int gx = (int)std::lround((other.pos3D.x - ref.pos3D.x) / pitch);
    const int gy = (int)std::lround((other.pos3D.y - ref.pos3D.y) / pitch);
    if (gx == 0 && gy == 0) throw Error(SVA_ERR_INVALID_ARG, "pairStep: cameras coincide");
    int a = std::abs(gx), b = std::abs(gy);
    while (b) { const int r = a % b; a = b; b = r; }
    PairStep s;
    s.dir = -gx / a;
    s.dir_y = -gy / a;
    s.k = std::max(std::abs(gx), std::abs(gy));
    s.baseline = s.k * pitch;
    return s;
}

// Mode S on an array pair: base parameters with the pair's step applied.
inline std::vector<uint16_t> computeDisparityPair(Engine& eng, const ImageView& ref,
                                                  const ImageView& other, const PairStep& step,
                                                  sva_sgm_params p) {
    p.dir = step.dir;
    p.dir_y = step.dir_y;
    return computeDisparitySGM(eng, ref, other, p);
}

// Median depth over the maps of one reference camera, f64,
// 0 where no map is valid.  maps[i] is W*H u16, baselines[i] its major-axis
// baseline (PairStep::baseline).
inline std::vector<double> fuseDepth(Engine& eng, const std::vector<std::vector<uint16_t>>& maps,
                                     int W, int H, const std::vector<double>& baselines, double f,
                                     double pixel_size, uint16_t invalid = 0xFFFF,
                                     std::vector<uint8_t>* n_valid = nullptr) {
    const size_t np = (size_t)W * H;
    if (maps.empty() || maps.size() != baselines.size())
        throw Error(SVA_ERR_INVALID_ARG, "fuseDepth: need one baseline per map");
    std::vector<uint16_t> packed(np * maps.size());
    for (size_t i = 0; i < maps.size(); i++) {
        if (maps[i].size() != np) throw Error(SVA_ERR_INVALID_ARG, "fuseDepth: map size");
        std::copy(maps[i].begin(), maps[i].end(), packed.begin() + i * np);
    }
    std::vector<double> depth(np);
    uint8_t* nv = nullptr;
    if (n_valid) {
        n_valid->resize(np);
        nv = n_valid->data();
    }
    eng.check(sva_fuse_depth(eng.handle(), packed.data(), (int)maps.size(), W, H,
                             baselines.data(), f, pixel_size, invalid, depth.data(), nv));
    return depth;
}

// ---- multi-GPU engine (sva.h "multi-GPU engine") ----------

// RAII owner of an sva_multi engine: pairs shard over `devices` (pair j ->
// devices[j mod n]) and over each device's streams; maps are gathered to
// devices[0] by RCCL (default) or peer copies (SVA_MULTI_GATHER_PEER).
class MultiEngine {
public:
    explicit MultiEngine(const std::vector<int>& devices, int streamsPerDevice = 2,
                         int flags = SVA_MULTI_GATHER_RCCL) {
        int s = sva_multi_create(devices.data(), (int)devices.size(), streamsPerDevice, flags, &m_);
        if (s != SVA_OK) throw Error(s, std::string("sva_multi_create: ") + sva_status_string(s));
    }
    ~MultiEngine() {
        if (m_) sva_multi_destroy(m_);
    }
    MultiEngine(const MultiEngine&) = delete;
    MultiEngine& operator=(const MultiEngine&) = delete;
    void* handle() const { return m_; }
    void check(int s) const {
        if (s != SVA_OK) throw Error(s, sva_multi_last_error(m_));
    }
    void synchronize() { check(sva_multi_synchronize(m_)); }

private:
    void* m_ = nullptr;
};

namespace detail {
// The C-ABI form of one camera-array frame, shared by the four
// computeArrayDepth*: the pairs grouped by reference camera (stable: the
// order reference cameras first appear in `pairs`), each with its grid step.
struct ArrayFrame {
    int W = 0, H = 0;
    size_t pitch = 0;
    std::vector<int> refs;                // reference camera of each group
    std::vector<sva_array_pair> ap;
    std::vector<int32_t> group_start;
    std::vector<size_t> order;            // ap index -> index in pairs
    std::vector<const uint8_t*> ptrs;

    // every pair's plane of `all` ([ap][H][W]) back in `pairs` order
    template <typename T>
    void scatter(const std::vector<T>& all, size_t n_pairs, std::vector<std::vector<T>>* out) const {
        const size_t np = (size_t)W * H;
        out->assign(n_pairs, {});
        for (size_t i = 0; i < ap.size(); i++)
            (*out)[order[i]].assign(all.begin() + i * np, all.begin() + (i + 1) * np);
    }
    // fn(handle, <the frame: images .. n_groups>, tail...): one of sva_array_depth*
    template <typename Fn, typename... Tail>
    int call(Fn fn, void* handle, Tail... tail) const {
        return fn(handle, ptrs.data(), (int)ptrs.size(), W, H, pitch, ap.data(), (int)ap.size(),
                  group_start.data(), (int)refs.size(), tail...);
    }
    template <typename T>
    std::vector<std::vector<T>> split(const std::vector<T>& planes) const {
        const size_t np = (size_t)W * H;
        std::vector<std::vector<T>> out(refs.size());
        for (size_t g = 0; g < refs.size(); g++)
            out[g].assign(planes.begin() + g * np, planes.begin() + (g + 1) * np);
        return out;
    }
};

inline ArrayFrame arrayFrame(const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
                             const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p,
                             double pitch, const char* who) {
    if (pairs.empty()) throw Error(SVA_ERR_INVALID_ARG, std::string(who) + ": no camera pairs");
    const ImageView& first = images.at(pairs[0][0]);
    ArrayFrame fr;
    fr.W = first.width;
    fr.H = first.height;
    fr.pitch = first.pitch;
    for (const auto& im : images)
        if (im.width != fr.W || im.height != fr.H || im.pitch != first.pitch)
            throw Error(SVA_ERR_INVALID_ARG, std::string(who) + ": images differ in size");
    for (const auto& pr : pairs)
        if (std::find(fr.refs.begin(), fr.refs.end(), pr[0]) == fr.refs.end())
            fr.refs.push_back(pr[0]);
    for (int r : fr.refs) {
        fr.group_start.push_back((int32_t)fr.ap.size());
        for (size_t j = 0; j < pairs.size(); j++) {
            if (pairs[j][0] != r) continue;
            const PairStep st = pairStep(cameras.at(pairs[j][0]), cameras.at(pairs[j][1]), pitch);
            sva_array_pair a;
            a.ref = pairs[j][0];
            a.other = pairs[j][1];
            a.params = p;
            a.params.dir = st.dir;
            a.params.dir_y = st.dir_y;
            a.baseline = st.baseline;
            fr.ap.push_back(a);
            fr.order.push_back(j);
        }
    }
    fr.group_start.push_back((int32_t)fr.ap.size());
    for (const auto& im : images) fr.ptrs.push_back(im.data);
    return fr;
}

// What computeArrayDepth, Conf, Multi and Mixed share around their one C call:
// the depth planes and, when asked for, the map planes -- one per pair (back in
// `pairs` order) or, per_group, one per reference camera.  call(f, pixel_size,
// depth, maps) makes the call with the first reference camera's f and
// pixel_size.
template <typename Call>
inline std::vector<std::vector<double>> arrayDepth(const ArrayFrame& fr,
                                                   const std::vector<Camera>& cameras,
                                                   size_t n_pairs, bool per_group,
                                                   std::vector<std::vector<uint16_t>>* maps,
                                                   const Call& call) {
    const size_t np = (size_t)fr.W * fr.H, ng = fr.refs.size();
    std::vector<double> depth(np * ng);
    std::vector<uint16_t> all(maps ? np * (per_group ? ng : fr.ap.size()) : 0);
    const Camera& c0 = cameras.at(fr.refs[0]);
    call(c0.f, c0.pixel_size, depth.data(), maps ? all.data() : nullptr);
    if (maps && per_group) *maps = fr.split(all);
    else if (maps) fr.scatter(all, n_pairs, maps);
    return fr.split(depth);
}

// The mixed route's unit baseline of every group: unit_k * pitch, or, with
// unit_k = 0, the group's largest baseline.
inline std::vector<double> unitBaselines(const ArrayFrame& fr, int unit_k, double pitch) {
    std::vector<double> unit(fr.refs.size());
    for (size_t g = 0; g < unit.size(); g++) {
        double u = unit_k * pitch;
        if (!unit_k)
            for (int j = fr.group_start[g]; j < fr.group_start[g + 1]; j++)
                u = std::max(u, fr.ap[j].baseline);
        unit[g] = u;
    }
    return unit;
}
}  // namespace detail

// One camera-array frame over a MultiEngine: replaces the pair loop of
// CameraStereoVision.cpp:55 for Mode S.  Every pair (getCameraPairs,
// functions.cpp:148-213) is matched along its own grid step (pairStep) with
// base parameters p; the maps of each reference camera are fused into one
// median depth map, in the order reference cameras first
// appear in `pairs`.  All images share width, height and pitch; f and
// pixel_size are the first reference camera's.  maps (nullable) receives
// every pair's u16 map in `pairs` order.
inline std::vector<std::vector<double>> computeArrayDepth(
    MultiEngine& m, const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
    const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p, double pitch = 0.05,
    std::vector<std::vector<uint16_t>>* maps = nullptr) {
    const detail::ArrayFrame fr = detail::arrayFrame(images, cameras, pairs, p, pitch,
                                                     "computeArrayDepth");
    return detail::arrayDepth(fr, cameras, pairs.size(), false, maps,
                              [&](double f, double pixel_size, double* depth, uint16_t* all) {
        m.check(fr.call(sva_array_depth, m.handle(), f, pixel_size, depth, nullptr, all));
    });
}

// computeArrayDepth with confidence (sva_array_depth_conf): the same grouping,
// every pair matched with the uniqueness filter (0..100, 0 = off), and each
// reference camera's maps fused by `mode`: SVA_FUSE_MIN_COST, SVA_FUSE_MAX_MARGIN
//  or SVA_FUSE_MEDIAN on the filtered maps.  winner (nullable;
// not with SVA_FUSE_MEDIAN) receives per group the chosen pair's index within
// the group, 0xFF where no map is valid.
inline std::vector<std::vector<double>> computeArrayDepthConf(
    MultiEngine& m, const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
    const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p, int uniqueness,
    int mode = SVA_FUSE_MIN_COST, double pitch = 0.05,
    std::vector<std::vector<uint16_t>>* maps = nullptr,
    std::vector<std::vector<uint8_t>>* winner = nullptr) {
    const detail::ArrayFrame fr = detail::arrayFrame(images, cameras, pairs, p, pitch,
                                                     "computeArrayDepthConf");
    std::vector<uint8_t> win(winner ? (size_t)fr.W * fr.H * fr.refs.size() : 0);
    auto out = detail::arrayDepth(fr, cameras, pairs.size(), false, maps,
                                  [&](double f, double pixel_size, double* depth, uint16_t* all) {
        m.check(fr.call(sva_array_depth_conf, m.handle(), f, pixel_size, uniqueness, mode, depth,
                        nullptr, winner ? win.data() : nullptr, all, nullptr, nullptr));
    });
    if (winner) *winner = fr.split(win);
    return out;
}

// ---- multi-baseline Mode S ----------------------

namespace detail {
// computeDisparityMulti (mixed false: the pairs share PairStep::k) and
// computeDisparityMixed (pair i enters at the ratio steps[i].k / unit_k).
inline std::vector<uint16_t> disparityMulti(
    Engine& eng, const std::string& who, const ImageView& ref,
    const std::vector<ImageView>& others, const std::vector<PairStep>& steps, bool mixed,
    int unit_k, const sva_sgm_params& p, int uniqueness, std::vector<float>* subpix,
    std::vector<uint16_t>* cost_min, std::vector<uint16_t>* cost_second) {
    if (others.empty() || others.size() != steps.size())
        throw Error(SVA_ERR_INVALID_ARG, who + ": need one step per matched image");
    if (mixed && unit_k < 1) throw Error(SVA_ERR_INVALID_ARG, who + ": unit_k must be >= 1");
    std::vector<const uint8_t*> ptrs;
    std::vector<int32_t> st, ratios;
    for (size_t i = 0; i < others.size(); i++) {
        const ImageView& o = others[i];
        if (o.width != ref.width || o.height != ref.height || o.pitch != ref.pitch)
            throw Error(SVA_ERR_INVALID_ARG, who + ": images differ in size");
        if (!mixed && steps[i].k != steps[0].k)
            throw Error(SVA_ERR_INVALID_ARG, who + ": pairs of unequal baselines");
        int a = steps[i].k, b = unit_k;
        while (b) { const int r = a % b; a = b; b = r; }
        if (mixed && a < 1) throw Error(SVA_ERR_INVALID_ARG, who + ": a step with k = 0");
        ptrs.push_back(o.data);
        st.push_back(steps[i].dir);
        st.push_back(steps[i].dir_y);
        if (mixed) {
            ratios.push_back(steps[i].k / a);
            ratios.push_back(unit_k / a);
        }
    }
    const size_t np = (size_t)ref.width * ref.height;
    std::vector<uint16_t> disp(np);
    float* sp = nullptr;
    if (subpix && p.subpixel) {
        subpix->resize(np);
        sp = subpix->data();
    }
    if (cost_min) cost_min->resize(np);
    if (cost_second) cost_second->resize(np);
    uint16_t* cmin = cost_min ? cost_min->data() : nullptr;
    uint16_t* csec = cost_second ? cost_second->data() : nullptr;
    const int n = (int)ptrs.size();
    eng.check(mixed ? sva_disparity_sgm_mixed(eng.handle(), ref.data, ptrs.data(), st.data(),
                                              ratios.data(), n, ref.width, ref.height, ref.pitch,
                                              &p, uniqueness, disp.data(), sp, cmin, csec)
                    : sva_disparity_sgm_multi(eng.handle(), ref.data, ptrs.data(), st.data(), n,
                                              ref.width, ref.height, ref.pitch, &p, uniqueness,
                                              disp.data(), sp, cmin, csec));
    return disp;
}
}  // namespace detail

// One reference image against several matched images, image i along steps[i]
// (PairStep of (ref, other_i); the pairs must share PairStep::k, so that one
// disparity is one depth in all of them): the pairs' cost volumes are fused
// before ONE aggregation (sva_disparity_sgm_multi).  p.dir / p.dir_y are
// ignored.  uniqueness 0..100 (0 = off); subpix, cost_min, cost_second are
// optional outputs as for sva_disparity_sgm_conf.
inline std::vector<uint16_t> computeDisparityMulti(
    Engine& eng, const ImageView& ref, const std::vector<ImageView>& others,
    const std::vector<PairStep>& steps, const sva_sgm_params& p, int uniqueness = 0,
    std::vector<float>* subpix = nullptr, std::vector<uint16_t>* cost_min = nullptr,
    std::vector<uint16_t>* cost_second = nullptr) {
    return detail::disparityMulti(eng, "computeDisparityMulti", ref, others, steps, false, 0, p,
                                  uniqueness, subpix, cost_min, cost_second);
}

// computeArrayDepth on the multi-baseline route (sva_array_depth_mb): the same
// grouping by reference camera, but each group's pairs are fused at the cost
// level and aggregated once, so there is ONE map per reference camera: depth =
// baseline * f / (d * pixel_size).  The pairs of a group must have equal
// major-axis baselines (e.g. a camera's 8 neighbours).  maps (nullable)
// receives each group's u16 map, in the order of the result.
inline std::vector<std::vector<double>> computeArrayDepthMulti(
    MultiEngine& m, const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
    const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p, int uniqueness = 0,
    double pitch = 0.05, std::vector<std::vector<uint16_t>>* maps = nullptr) {
    const detail::ArrayFrame fr = detail::arrayFrame(images, cameras, pairs, p, pitch,
                                                     "computeArrayDepthMulti");
    return detail::arrayDepth(fr, cameras, pairs.size(), true, maps,
                              [&](double f, double pixel_size, double* depth, uint16_t* all) {
        m.check(fr.call(sva_array_depth_mb, m.handle(), f, pixel_size, uniqueness, depth, all,
                        nullptr, nullptr));
    });
}

// computeDisparityMulti for pairs of UNEQUAL baselines (sva_disparity_sgm_mixed):
// disparity counts pixels of a pair whose PairStep::k is unit_k, and pair i
// enters at the ratio steps[i].k / unit_k (num and den in 1..8 once reduced;
// the library refuses anything else).  Depth: unit_k * pitch * f / (d *
// pixel_size).
inline std::vector<uint16_t> computeDisparityMixed(
    Engine& eng, const ImageView& ref, const std::vector<ImageView>& others,
    const std::vector<PairStep>& steps, int unit_k, const sva_sgm_params& p, int uniqueness = 0,
    std::vector<float>* subpix = nullptr, std::vector<uint16_t>* cost_min = nullptr,
    std::vector<uint16_t>* cost_second = nullptr) {
    return detail::disparityMulti(eng, "computeDisparityMixed", ref, others, steps, true, unit_k,
                                  p, uniqueness, subpix, cost_min, cost_second);
}

// computeArrayDepthMulti for groups of unequal baselines (sva_array_depth_mixed):
// every pair of a reference camera, whatever its baseline, in ONE fused volume.
// unit_k: the PairStep::k that a group's disparity counts pixels of; 0 = each
// group's largest k (the finest depth resolution).  Each pair's k / unit_k must
// reduce to num/den in 1..8.
inline std::vector<std::vector<double>> computeArrayDepthMixed(
    MultiEngine& m, const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
    const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p, int unit_k = 0,
    int uniqueness = 0, double pitch = 0.05, std::vector<std::vector<uint16_t>>* maps = nullptr) {
    if (unit_k < 0) throw Error(SVA_ERR_INVALID_ARG, "computeArrayDepthMixed: unit_k must be >= 0");
    const detail::ArrayFrame fr = detail::arrayFrame(images, cameras, pairs, p, pitch,
                                                     "computeArrayDepthMixed");
    const std::vector<double> unit = detail::unitBaselines(fr, unit_k, pitch);
    return detail::arrayDepth(fr, cameras, pairs.size(), true, maps,
                              [&](double f, double pixel_size, double* depth, uint16_t* all) {
        m.check(fr.call(sva_array_depth_mixed, m.handle(), (const double*)unit.data(), f,
                        pixel_size, uniqueness, depth, all, nullptr, nullptr));
    });
}

// ---- sub-pixel depth -----------------------------------

namespace detail {
inline void packMaps(const char* who, const std::vector<std::vector<uint16_t>>& maps,
                     const std::vector<std::vector<float>>& subpix, size_t np, size_t n_baselines,
                     std::vector<uint16_t>* d, std::vector<float>* s) {
    if (maps.empty() || maps.size() != n_baselines || subpix.size() != maps.size())
        throw Error(SVA_ERR_INVALID_ARG,
                    std::string(who) + ": need one baseline and one sub-pixel map per map");
    d->resize(np * maps.size());
    s->resize(np * maps.size());
    for (size_t i = 0; i < maps.size(); i++) {
        if (maps[i].size() != np || subpix[i].size() != np)
            throw Error(SVA_ERR_INVALID_ARG, std::string(who) + ": map size");
        std::copy(maps[i].begin(), maps[i].end(), d->begin() + i * np);
        std::copy(subpix[i].begin(), subpix[i].end(), s->begin() + i * np);
    }
}
}  // namespace detail

// fuseDepth on the f32 sub-pixel maps the matchers write next to the u16 ones
// (computeDisparitySGM's subpix): depth is no longer quantised to whole
// disparities.  A map counts where its u16 disparity is valid and its
// sub-pixel disparity is > 0 (NaN, a rejected pixel, is not).
inline std::vector<double> fuseDepthSub(Engine& eng, const std::vector<std::vector<uint16_t>>& maps,
                                        const std::vector<std::vector<float>>& subpix, int W, int H,
                                        const std::vector<double>& baselines, double f,
                                        double pixel_size, uint16_t invalid = 0xFFFF,
                                        std::vector<uint8_t>* n_valid = nullptr) {
    const size_t np = (size_t)W * H;
    std::vector<uint16_t> d;
    std::vector<float> s;
    detail::packMaps("fuseDepthSub", maps, subpix, np, baselines.size(), &d, &s);
    std::vector<double> depth(np);
    if (n_valid) n_valid->resize(np);
    eng.check(sva_fuse_depth_sub(eng.handle(), d.data(), s.data(), (int)maps.size(), W, H,
                                 baselines.data(), f, pixel_size, invalid, depth.data(),
                                 n_valid ? n_valid->data() : nullptr));
    return depth;
}

// Cost-aware fusion with the winner's depth from its
// sub-pixel map: mode SVA_FUSE_MIN_COST (cost_second may be empty) or
// SVA_FUSE_MAX_MARGIN.  winner (nullable): the chosen map's index, 0xFF if none.
inline std::vector<double> fuseDepthConfSub(
    Engine& eng, const std::vector<std::vector<uint16_t>>& maps,
    const std::vector<std::vector<float>>& subpix,
    const std::vector<std::vector<uint16_t>>& cost_min,
    const std::vector<std::vector<uint16_t>>& cost_second, int W, int H,
    const std::vector<double>& baselines, double f, double pixel_size, int mode,
    uint16_t invalid = 0xFFFF, std::vector<uint8_t>* n_valid = nullptr,
    std::vector<uint8_t>* winner = nullptr) {
    const size_t np = (size_t)W * H;
    std::vector<uint16_t> d, cmin, csec;
    std::vector<float> s;
    detail::packMaps("fuseDepthConfSub", maps, subpix, np, baselines.size(), &d, &s);
    if (cost_min.size() != maps.size() || (!cost_second.empty() && cost_second.size() != maps.size()))
        throw Error(SVA_ERR_INVALID_ARG, "fuseDepthConfSub: need one cost plane per map");
    for (size_t i = 0; i < maps.size(); i++) {
        if (cost_min[i].size() != np || (!cost_second.empty() && cost_second[i].size() != np))
            throw Error(SVA_ERR_INVALID_ARG, "fuseDepthConfSub: cost plane size");
        cmin.insert(cmin.end(), cost_min[i].begin(), cost_min[i].end());
        if (!cost_second.empty()) csec.insert(csec.end(), cost_second[i].begin(), cost_second[i].end());
    }
    std::vector<double> depth(np);
    if (n_valid) n_valid->resize(np);
    if (winner) winner->resize(np);
    eng.check(sva_fuse_depth_conf_sub(eng.handle(), d.data(), s.data(), cmin.data(),
                                      csec.empty() ? nullptr : csec.data(), (int)maps.size(), W, H,
                                      baselines.data(), f, pixel_size, invalid, mode, depth.data(),
                                      n_valid ? n_valid->data() : nullptr,
                                      winner ? winner->data() : nullptr));
    return depth;
}

// Sub-pixel depth from one camera-array frame (sva_array_depth_sub): the frame
// of computeArrayDepthConf (route SVA_ARRAY_PAIRS; mode as there),
// computeArrayDepthMulti (SVA_ARRAY_GROUPS) or computeArrayDepthMixed
// (SVA_ARRAY_GROUPS_MIXED, with its unit_k), every job matched with
// subpixel = 1 and depth fused from the f32 maps.  On the group routes mode
// must stay SVA_FUSE_MEDIAN.  maps (nullable) as for the entry of that route:
// one per pair in `pairs` order, or one per reference camera.
inline std::vector<std::vector<double>> computeArrayDepthSub(
    MultiEngine& m, const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
    const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p,
    int route = SVA_ARRAY_PAIRS, int uniqueness = 0, int mode = SVA_FUSE_MEDIAN, int unit_k = 0,
    double pitch = 0.05, std::vector<std::vector<uint16_t>>* maps = nullptr) {
    if (unit_k < 0) throw Error(SVA_ERR_INVALID_ARG, "computeArrayDepthSub: unit_k must be >= 0");
    const detail::ArrayFrame fr = detail::arrayFrame(images, cameras, pairs, p, pitch,
                                                     "computeArrayDepthSub");
    std::vector<double> unit;
    if (route == SVA_ARRAY_GROUPS_MIXED) unit = detail::unitBaselines(fr, unit_k, pitch);
    return detail::arrayDepth(fr, cameras, pairs.size(), route != SVA_ARRAY_PAIRS, maps,
                              [&](double f, double pixel_size, double* depth, uint16_t* all) {
        m.check(fr.call(sva_array_depth_sub, m.handle(), route,
                        unit.empty() ? (const double*)nullptr : (const double*)unit.data(), f,
                        pixel_size, uniqueness, mode, depth, (uint8_t*)nullptr, (uint8_t*)nullptr,
                        (float*)nullptr, all, (uint16_t*)nullptr, (uint16_t*)nullptr));
    });
}

// ---- the post-filter chain: what its filters and frames share ---------------

namespace detail {
// The packing the four map filters share: maps[i] (W*H u16 each) and, unless
// empty, subpix[i] back to back as the C calls take them.  need: what is thrown
// when there is no map, or not one sub-pixel map per map.
struct PackedMaps {
    size_t np = 0, n = 0;
    std::vector<uint16_t> d;
    std::vector<float> s;
    float* sub() { return s.empty() ? nullptr : s.data(); }
};
inline PackedMaps packFilterMaps(const std::string& who, const char* need,
                                 const std::vector<std::vector<uint16_t>>& maps,
                                 const std::vector<std::vector<float>>& subpix, int W, int H) {
    PackedMaps p;
    p.np = (size_t)W * H;
    p.n = maps.size();
    if (maps.empty() || (!subpix.empty() && subpix.size() != p.n))
        throw Error(SVA_ERR_INVALID_ARG, who + ": " + need);
    p.d.resize(p.np * p.n);
    p.s.resize(subpix.empty() ? 0 : p.np * p.n);
    for (size_t i = 0; i < p.n; i++) {
        if (maps[i].size() != p.np || (!subpix.empty() && subpix[i].size() != p.np))
            throw Error(SVA_ERR_INVALID_ARG, who + ": map size");
        std::copy(maps[i].begin(), maps[i].end(), p.d.begin() + i * p.np);
        if (!subpix.empty()) std::copy(subpix[i].begin(), subpix[i].end(), p.s.begin() + i * p.np);
    }
    return p;
}

// n planes of np back to back, one vector each (nothing of an empty `all`).
template <typename T>
inline std::vector<std::vector<T>> unpackPlanes(const std::vector<T>& all, size_t np, size_t n) {
    std::vector<std::vector<T>> out;
    for (size_t i = 0; i < n && !all.empty(); i++)
        out.emplace_back(all.begin() + i * np, all.begin() + (i + 1) * np);
    return out;
}

// What the post-filter chain's frames (computeArrayDepthChecked, Filtered,
// Filled, Smoothed) share around their one C call.  Every camera's view_step is
// minus its grid offset from cameras[0], in units of `pitch`, and the mixed
// route's unit baseline is `pitch`.
struct ChainFrame {
    ArrayFrame fr;
    size_t n_pairs;
    bool per_group;                  // one job per reference camera, else per pair
    std::vector<double> unit;
    std::vector<int32_t> vs;

    ChainFrame(const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
               const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p, int route,
               double pitch, const char* who)
        : fr(arrayFrame(images, cameras, pairs, p, pitch, who)), n_pairs(pairs.size()),
          per_group(route != SVA_ARRAY_PAIRS) {
        if (route == SVA_ARRAY_GROUPS_MIXED) unit = unitBaselines(fr, 1, pitch);
        for (const Camera& c : cameras) {
            vs.push_back(-(int32_t)std::lround((c.pos3D.x - cameras[0].pos3D.x) / pitch));
            vs.push_back(-(int32_t)std::lround((c.pos3D.y - cameras[0].pos3D.y) / pitch));
        }
    }
    // A stage's per-job plane: its storage (empty unless asked for), what the C
    // call takes, and the planes given back per reference camera or in `pairs` order.
    template <typename T>
    std::vector<T> plane(const std::vector<std::vector<T>>* asked) const {
        return std::vector<T>(asked ? (size_t)fr.W * fr.H * (per_group ? fr.refs.size() : fr.ap.size())
                                    : 0);
    }
    template <typename T>
    static T* ptr(std::vector<T>& all) { return all.empty() ? nullptr : all.data(); }
    template <typename T>
    void give(const std::vector<T>& all, std::vector<std::vector<T>>* asked) const {
        if (asked && per_group) *asked = fr.split(all);
        else if (asked) fr.scatter(all, n_pairs, asked);
    }
    // fn: one of the chain's entries; its arguments from `route` to the check's
    // conflict plane, every optional plane but maps left out, then tail...
    template <typename Fn, typename... Tail>
    std::vector<std::vector<double>> depth(MultiEngine& m, const std::vector<Camera>& cameras, Fn fn,
                                           int route, int uniqueness, int mode,
                                           std::vector<std::vector<uint16_t>>* maps, bool sub,
                                           int max_diff, int min_agree, int max_conflict,
                                           uint8_t* agree, uint8_t* conflict, Tail... tail) const {
        return arrayDepth(fr, cameras, n_pairs, per_group, maps,
                          [&](double f, double pixel_size, double* depth, uint16_t* all) {
            m.check(fr.call(fn, m.handle(), route,
                            unit.empty() ? (const double*)nullptr : (const double*)unit.data(), f,
                            pixel_size, uniqueness, mode, depth, (uint8_t*)nullptr, (uint8_t*)nullptr,
                            (float*)nullptr, all, (uint16_t*)nullptr, (uint16_t*)nullptr,
                            (const int32_t*)vs.data(), sub ? 1 : 0, max_diff, min_agree, max_conflict,
                            agree, conflict, tail...));
        });
    }
};
}  // namespace detail

// ---- cross-view consistency check ------------------------

// What crossCheck keeps of each view: the checked map, and the optional planes.
struct CrossChecked {
    std::vector<std::vector<uint16_t>> maps;
    std::vector<std::vector<float>> subpix;       // empty unless sub-pixel maps went in
    std::vector<std::vector<uint8_t>> agree, conflict;
};

// The consistency test between the maps of several reference cameras
// (sva_cross_check): maps[v] is W*H u16 and counts pixels of one unit baseline
// shared by all views, view_step[v] is view v's position in unit baselines in
// the sense of PairStep (dir, dir_y) -- minus its grid offset.  A valid pixel
// stays where at least min_agree other views hold a disparity within max_diff
// at the pixel that sees the same point, and at most max_conflict hold a smaller
// one (they see through it); otherwise it becomes `invalid`, and NaN in subpix.
// subpix: empty, or one f32 map per view.
inline CrossChecked crossCheck(Engine& eng, const std::vector<std::vector<uint16_t>>& maps,
                               const std::vector<std::vector<float>>& subpix, int W, int H,
                               const std::vector<std::array<int32_t, 2>>& view_step,
                               int max_diff = 1, int min_agree = 1, int max_conflict = 0,
                               uint16_t invalid = 0xFFFF) {
    const char* need = "need one view_step (and sub-pixel map) per map";
    if (view_step.size() != maps.size())
        throw Error(SVA_ERR_INVALID_ARG, std::string("crossCheck: ") + need);
    detail::PackedMaps in = detail::packFilterMaps("crossCheck", need, maps, subpix, W, H);
    const size_t np = in.np, n = in.n;
    std::vector<uint16_t> out(np * n);
    std::vector<float> out_s(in.s.size());
    std::vector<uint8_t> ag(np * n), cf(np * n);
    std::vector<int32_t> vs;
    for (const auto& v : view_step) vs.insert(vs.end(), {v[0], v[1]});
    eng.check(sva_cross_check(eng.handle(), in.d.data(), in.sub(), (int)n, W, H, vs.data(), invalid,
                              max_diff, min_agree, max_conflict, out.data(),
                              in.s.empty() ? nullptr : out_s.data(), ag.data(), cf.data()));
    return {detail::unpackPlanes(out, np, n), detail::unpackPlanes(out_s, np, n),
            detail::unpackPlanes(ag, np, n), detail::unpackPlanes(cf, np, n)};
}

// computeArrayDepthMulti / Mixed (sub = false) or the group routes of
// computeArrayDepthSub (sub = true) with the cross-view check between the
// reference cameras' maps before depth (sva_array_depth_checked).  route:
// SVA_ARRAY_GROUPS or SVA_ARRAY_GROUPS_MIXED.  Every camera's view_step is
// minus its grid offset from cameras[0], in units of `pitch`; on
// SVA_ARRAY_GROUPS the pairs must therefore be one grid unit long on their
// major axis, and on GROUPS_MIXED the unit baseline is `pitch` (a longer unit
// would put the cameras at fractions of it, which view_step cannot say).
// maps, agree, conflict (nullable): one plane per reference camera, in the
// order of the result.
inline std::vector<std::vector<double>> computeArrayDepthChecked(
    MultiEngine& m, const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
    const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p,
    int route = SVA_ARRAY_GROUPS, bool sub = false, int max_diff = 1, int min_agree = 1,
    int max_conflict = 0, int uniqueness = 0, double pitch = 0.05,
    std::vector<std::vector<uint16_t>>* maps = nullptr,
    std::vector<std::vector<uint8_t>>* agree = nullptr,
    std::vector<std::vector<uint8_t>>* conflict = nullptr) {
    const detail::ChainFrame cf(images, cameras, pairs, p, route, pitch, "computeArrayDepthChecked");
    const size_t planes = (size_t)cf.fr.W * cf.fr.H * cf.fr.refs.size();
    std::vector<uint8_t> ag(agree ? planes : 0), cn(conflict ? planes : 0);
    auto depth = cf.depth(m, cameras, sva_array_depth_checked, route, uniqueness,
                          (int)SVA_FUSE_MEDIAN, maps, sub, max_diff, min_agree, max_conflict,
                          cf.ptr(ag), cf.ptr(cn));
    if (agree) *agree = cf.fr.split(ag);
    if (conflict) *conflict = cf.fr.split(cn);
    return depth;
}

// ---- speckle filter ---------------------------------------

// What filterSpeckles keeps of each map: the filtered map, the optional f32
// map, and the size of every pixel's component (0 where the pixel is not valid).
struct SpeckleFiltered {
    std::vector<std::vector<uint16_t>> maps;
    std::vector<std::vector<float>> subpix;       // empty unless sub-pixel maps went in
    std::vector<std::vector<uint32_t>> comp_size;
};

// Removes the small connected components of each map (sva_filter_speckles): a
// valid pixel (not `invalid`, not 0) whose 4-connected component -- neighbours
// linked where both are valid and differ by at most max_diff -- has at most
// max_size pixels becomes `invalid`, and NaN in subpix.  maps[i] is W*H u16;
// subpix: empty, or one f32 map per map.  max_size = 0 returns the input.
inline SpeckleFiltered filterSpeckles(Engine& eng, const std::vector<std::vector<uint16_t>>& maps,
                                      const std::vector<std::vector<float>>& subpix, int W, int H,
                                      int max_size, int max_diff, uint16_t invalid = 0xFFFF) {
    detail::PackedMaps io = detail::packFilterMaps("filterSpeckles", "need one sub-pixel map per map",
                                                   maps, subpix, W, H);
    std::vector<uint32_t> size(io.np * io.n);
    // in place on the packed copies
    eng.check(sva_filter_speckles(eng.handle(), io.d.data(), io.sub(), (int)io.n, W, H, invalid,
                                  max_size, max_diff, io.d.data(), io.sub(), size.data()));
    return {detail::unpackPlanes(io.d, io.np, io.n), detail::unpackPlanes(io.s, io.np, io.n),
            detail::unpackPlanes(size, io.np, io.n)};
}

// An array frame with the speckle filter over every job's map before depth
// (sva_array_depth_filtered).  check = false: the frame of computeArrayDepthConf
// (route SVA_ARRAY_PAIRS; mode as there, per-pair lr_check allowed),
// computeArrayDepthMulti (SVA_ARRAY_GROUPS) or computeArrayDepthMixed
// (SVA_ARRAY_GROUPS_MIXED, unit baseline `pitch`), or with sub = true of
// computeArrayDepthSub.  check = true: computeArrayDepthChecked (group routes,
// its view_step convention and thresholds), the filter after the check.
// maps, comp_size (nullable): one plane per pair in `pairs` order, or one per
// reference camera.
inline std::vector<std::vector<double>> computeArrayDepthFiltered(
    MultiEngine& m, const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
    const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p, int speckle_max_size,
    int speckle_max_diff, int route = SVA_ARRAY_GROUPS, bool check = false, bool sub = false,
    int max_diff = 1, int min_agree = 1, int max_conflict = 0, int uniqueness = 0,
    int mode = SVA_FUSE_MEDIAN, double pitch = 0.05,
    std::vector<std::vector<uint16_t>>* maps = nullptr,
    std::vector<std::vector<uint32_t>>* comp_size = nullptr) {
    const detail::ChainFrame cf(images, cameras, pairs, p, route, pitch, "computeArrayDepthFiltered");
    std::vector<uint32_t> size = cf.plane(comp_size);
    auto depth = cf.depth(m, cameras, sva_array_depth_filtered, route, uniqueness, mode, maps, sub,
                          max_diff, min_agree, max_conflict, (uint8_t*)nullptr, (uint8_t*)nullptr,
                          check ? 1 : 0, speckle_max_size, speckle_max_diff, cf.ptr(size));
    cf.give(size, comp_size);
    return depth;
}

// ---- hole filling -----------------------------------------

// What fillHoles makes of each map: the filled map, the optional f32 map, and
// the number of directions that found a valid pixel (0 where the pixel is valid).
struct HolesFilled {
    std::vector<std::vector<uint16_t>> maps;
    std::vector<std::vector<float>> subpix;       // empty unless sub-pixel maps went in
    std::vector<std::vector<uint8_t>> n_found;
};

// Fills the holes of each map (sva_fill_holes): a pixel that is 0 or `invalid`
// looks up to max_dist steps along the eight directions for the nearest valid
// pixel of the input map; with at least min_found candidates it takes the one
// `mode` picks of them sorted by (value, distance, direction) -- SVA_FILL_MIN,
// SVA_FILL_SECOND (the occlusion rule) or SVA_FILL_MEDIAN -- and in subpix that
// source's f32 value.  maps[i] is W*H u16; subpix: empty, or one f32 map per
// map.  max_dist in 0..255; 0 returns the input.
inline HolesFilled fillHoles(Engine& eng, const std::vector<std::vector<uint16_t>>& maps,
                             const std::vector<std::vector<float>>& subpix, int W, int H,
                             int max_dist, int min_found = 1, int mode = SVA_FILL_SECOND,
                             uint16_t invalid = 0xFFFF) {
    detail::PackedMaps io = detail::packFilterMaps("fillHoles", "need one sub-pixel map per map",
                                                   maps, subpix, W, H);
    std::vector<uint8_t> found(io.np * io.n);
    // in place on the packed copies
    eng.check(sva_fill_holes(eng.handle(), io.d.data(), io.sub(), (int)io.n, W, H, invalid, max_dist,
                             min_found, mode, io.d.data(), io.sub(), found.data()));
    return {detail::unpackPlanes(io.d, io.np, io.n), detail::unpackPlanes(io.s, io.np, io.n),
            detail::unpackPlanes(found, io.np, io.n)};
}

// computeArrayDepthFiltered's frame with hole filling over every job's map
// after the speckle filter and before depth (sva_array_depth_filled).  The
// frame's cost planes stay the matcher's -- at a filled pixel they describe the
// rejected match -- so the median is the fusion mode that makes sense after a
// fill.  maps, n_found (nullable): one plane per pair in `pairs` order, or one
// per reference camera.
inline std::vector<std::vector<double>> computeArrayDepthFilled(
    MultiEngine& m, const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
    const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p, int fill_max_dist,
    int fill_min_found = 1, int fill_mode = SVA_FILL_SECOND, int speckle_max_size = 0,
    int speckle_max_diff = 0, int route = SVA_ARRAY_GROUPS, bool check = false, bool sub = false,
    int max_diff = 1, int min_agree = 1, int max_conflict = 0, int uniqueness = 0,
    int mode = SVA_FUSE_MEDIAN, double pitch = 0.05,
    std::vector<std::vector<uint16_t>>* maps = nullptr,
    std::vector<std::vector<uint8_t>>* n_found = nullptr) {
    const detail::ChainFrame cf(images, cameras, pairs, p, route, pitch, "computeArrayDepthFilled");
    std::vector<uint8_t> found = cf.plane(n_found);
    auto depth = cf.depth(m, cameras, sva_array_depth_filled, route, uniqueness, mode, maps, sub,
                          max_diff, min_agree, max_conflict, (uint8_t*)nullptr, (uint8_t*)nullptr,
                          check ? 1 : 0, speckle_max_size, speckle_max_diff, (uint32_t*)nullptr,
                          fill_max_dist, fill_min_found, fill_mode, cf.ptr(found));
    cf.give(found, n_found);
    return depth;
}

// ---- weighted median filter --------------------------------

// The weight table of weightedMedian for an intensity scale sigma > 0: entry i =
// lround(1024 * exp(-i / sigma)), so equal intensities weigh 1024 and a
// difference of about 7 sigma and more weighs nothing.
inline std::array<uint16_t, 256> wmedWeights(double sigma) {
    if (!(sigma > 0)) throw Error(SVA_ERR_INVALID_ARG, "wmedWeights: sigma must be positive");
    std::array<uint16_t, 256> w{};
    for (int i = 0; i < 256; i++) w[i] = (uint16_t)std::lround(1024.0 * std::exp(-i / sigma));
    return w;
}

// What weightedMedian makes of each map: the filtered map, the optional f32 map,
// and the number of candidates in the window (0 where the pixel was not looked at).
struct MedianFiltered {
    std::vector<std::vector<uint16_t>> maps;
    std::vector<std::vector<float>> subpix;       // empty unless sub-pixel maps went in
    std::vector<std::vector<uint16_t>> support;
};

// The weighted median filter of each map (sva_weighted_median): a pixel takes
// the lower weighted median of the valid pixels of its (2 * radius + 1)^2
// window, each weighted by weights[|guide(p) - guide(q)|], if at least
// min_support of them carry weight; in subpix the source pixel's f32 value.
// guides: empty (then weights must be null: the plain median over the valid
// pixels), or one W x H view per map, all of one pitch.  select: empty, or one
// u8 plane per map -- only its non-zero pixels are looked at.  fill = true also
// gives holes a value.  maps[i] is W*H u16.
inline MedianFiltered weightedMedian(Engine& eng, const std::vector<std::vector<uint16_t>>& maps,
                                     const std::vector<std::vector<float>>& subpix,
                                     const std::vector<ImageView>& guides,
                                     const std::array<uint16_t, 256>* weights, int W, int H,
                                     int radius, int min_support = 1, bool fill = true,
                                     const std::vector<std::vector<uint8_t>>& select = {},
                                     uint16_t invalid = 0xFFFF) {
    const size_t np = (size_t)W * H, n = maps.size();
    const char* need = "need one plane per map";
    if ((!guides.empty() && guides.size() != n) || (!select.empty() && select.size() != n))
        throw Error(SVA_ERR_INVALID_ARG, std::string("weightedMedian: ") + need);
    detail::PackedMaps in = detail::packFilterMaps("weightedMedian", need, maps, subpix, W, H);
    std::vector<uint8_t> sel;
    std::vector<const uint8_t*> g;
    for (size_t i = 0; i < n; i++) {
        if (!select.empty() && select[i].size() != np)
            throw Error(SVA_ERR_INVALID_ARG, "weightedMedian: map size");
        if (!select.empty()) sel.insert(sel.end(), select[i].begin(), select[i].end());
        if (guides.empty()) continue;
        if (guides[i].width != W || guides[i].height != H || guides[i].pitch != guides[0].pitch)
            throw Error(SVA_ERR_INVALID_ARG, "weightedMedian: guide size or pitch");
        g.push_back(guides[i].data);
    }
    std::vector<uint16_t> out(np * n), sup(np * n);
    std::vector<float> os(in.s.size());
    eng.check(sva_weighted_median(eng.handle(), in.d.data(), in.sub(), g.empty() ? nullptr : g.data(),
                                  g.empty() ? 0 : guides[0].pitch,
                                  weights ? weights->data() : nullptr,
                                  sel.empty() ? nullptr : sel.data(), (int)n, W, H, invalid, radius,
                                  min_support, fill ? 1 : 0, out.data(),
                                  in.s.empty() ? nullptr : os.data(), sup.data()));
    return {detail::unpackPlanes(out, np, n), detail::unpackPlanes(os, np, n),
            detail::unpackPlanes(sup, np, n)};
}

// computeArrayDepthFilled's frame with the weighted median filter over every
// job's map after the fill and before depth (sva_array_depth_smoothed), guided
// by the job's reference view; weights null: the unguided median.  wmed_select
// false filters every pixel, true only those the fill looked at.  maps, support
// (nullable): one plane per pair in `pairs` order, or one per reference camera.
inline std::vector<std::vector<double>> computeArrayDepthSmoothed(
    MultiEngine& m, const std::vector<ImageView>& images, const std::vector<Camera>& cameras,
    const std::vector<std::array<int, 2>>& pairs, const sva_sgm_params& p, int wmed_radius,
    const std::array<uint16_t, 256>* weights, int wmed_min_support = 1, bool wmed_select = false,
    int fill_max_dist = 0, int fill_min_found = 1, int fill_mode = SVA_FILL_SECOND,
    int speckle_max_size = 0, int speckle_max_diff = 0, int route = SVA_ARRAY_GROUPS,
    bool check = false, bool sub = false, int max_diff = 1, int min_agree = 1,
    int max_conflict = 0, int uniqueness = 0, int mode = SVA_FUSE_MEDIAN, double pitch = 0.05,
    std::vector<std::vector<uint16_t>>* maps = nullptr,
    std::vector<std::vector<uint16_t>>* support = nullptr) {
    const detail::ChainFrame cf(images, cameras, pairs, p, route, pitch, "computeArrayDepthSmoothed");
    std::vector<uint16_t> sup = cf.plane(support);
    auto depth = cf.depth(m, cameras, sva_array_depth_smoothed, route, uniqueness, mode, maps, sub,
                          max_diff, min_agree, max_conflict, (uint8_t*)nullptr, (uint8_t*)nullptr,
                          check ? 1 : 0, speckle_max_size, speckle_max_diff, (uint32_t*)nullptr,
                          fill_max_dist, fill_min_found, fill_mode, (uint8_t*)nullptr, wmed_radius,
                          weights ? weights->data() : (const uint16_t*)nullptr, wmed_min_support,
                          wmed_select ? 1 : 0, cf.ptr(sup));
    cf.give(sup, support);
    return depth;
}

// ---- rectification ----------------------------------

// The view of a calibration (sva_rectify_view_of; host only): h = K_raw . R .
// K_ideal^-1 with R taking ideal-camera rays to raw-camera rays, all row-major
// 3x3; dist = {k1, k2, p1, p2, k3}.  Throws on a K_raw with skew or a bottom row
// other than 0 0 1, a singular K_ideal or non-finite input.
inline sva_rectify_view rectifyViewOf(const std::array<double, 9>& K_raw,
                                      const std::array<double, 5>& dist,
                                      const std::array<double, 9>& R,
                                      const std::array<double, 9>& K_ideal) {
    sva_rectify_view v;
    if (int st = sva_rectify_view_of(K_raw.data(), dist.data(), R.data(), K_ideal.data(), &v))
        throw Error(st, "rectifyViewOf: bad calibration");
    return v;
}

// What rectifyViews makes of each raw view: the rectified view (out_w * out_h u8),
// its valid plane and, if asked for, the source position of every pixel in 1/32
// px as (qx, qy) pairs (INT32_MIN where the pixel looks outside the limits).
struct Rectified {
    std::vector<std::vector<uint8_t>> views, valid;
    std::vector<std::vector<int32_t>> map;        // empty unless asked for
};

// Warps raw views of one size onto the ideal grid (sva_rectify), view i by
// rect[i].  out_w, out_h 0: the source's size.  A pixel whose taps leave the
// source takes `border` there and is not valid.
inline Rectified rectifyViews(Engine& eng, const std::vector<ImageView>& raw,
                              const std::vector<sva_rectify_view>& rect, int out_w = 0,
                              int out_h = 0, int border = 0, bool want_map = false) {
    const size_t n = raw.size();
    if (n == 0 || rect.size() != n)
        throw Error(SVA_ERR_INVALID_ARG, "rectifyViews: need one sva_rectify_view per view");
    const int sw = raw[0].width, sh = raw[0].height;
    const int W = out_w ? out_w : sw, H = out_h ? out_h : sh;
    std::vector<uint8_t> src((size_t)sw * sh * n);
    for (size_t i = 0; i < n; i++) {
        if (raw[i].width != sw || raw[i].height != sh)
            throw Error(SVA_ERR_INVALID_ARG, "rectifyViews: view size");
        for (int y = 0; y < sh; y++)
            std::copy(raw[i].data + (size_t)y * raw[i].pitch, raw[i].data + (size_t)y * raw[i].pitch + sw,
                      src.begin() + (i * sh + y) * sw);
    }
    const size_t np = (size_t)W * H;
    std::vector<uint8_t> out(np * n), valid(np * n);
    std::vector<int32_t> map(want_map ? np * n * 2 : 0);
    eng.check(sva_rectify(eng.handle(), src.data(), (int)n, sw, sh, (size_t)sw, rect.data(), W, H,
                          (size_t)W, border, out.data(), valid.data(),
                          want_map ? map.data() : nullptr));
    return {detail::unpackPlanes(out, np, n), detail::unpackPlanes(valid, np, n),
            detail::unpackPlanes(map, np * 2, n)};
}

// What maskMaps keeps of each map.
struct MaskedMaps {
    std::vector<std::vector<uint16_t>> maps;
    std::vector<std::vector<float>> subpix;       // empty unless sub-pixel maps went in
};

// maps[i] takes `invalid`, and subpix[i] NaN, where valid[i] is 0 (sva_mask_maps):
// what a rectified reference view's valid plane says about its disparity map.
inline MaskedMaps maskMaps(Engine& eng, const std::vector<std::vector<uint16_t>>& maps,
                           const std::vector<std::vector<float>>& subpix,
                           const std::vector<std::vector<uint8_t>>& valid, int W, int H,
                           uint16_t invalid = 0xFFFF) {
    const char* need = "need one valid plane, and none or one sub-pixel map, per map";
    detail::PackedMaps io = detail::packFilterMaps("maskMaps", need, maps, subpix, W, H);
    if (valid.size() != io.n) throw Error(SVA_ERR_INVALID_ARG, std::string("maskMaps: ") + need);
    std::vector<uint8_t> v;
    for (const auto& plane : valid) {
        if (plane.size() != io.np) throw Error(SVA_ERR_INVALID_ARG, "maskMaps: map size");
        v.insert(v.end(), plane.begin(), plane.end());
    }
    eng.check(sva_mask_maps(eng.handle(), io.d.data(), io.sub(), (int)io.n, W, H, v.data(), invalid,
                            io.d.data(), io.sub()));
    return {detail::unpackPlanes(io.d, io.np, io.n), detail::unpackPlanes(io.s, io.np, io.n)};
}

// computeArrayDepthSmoothed's frame from RAW views (sva_array_depth_rectified):
// every device rectifies the views it needs by rect (one per image) before its
// jobs, and with mask every job's map is masked by its reference view's valid
// plane before the cross-view check.  wmed_radius 0 switches the weighted median
// off.  views, valid (nullable): the rectified views and their valid planes, one
// per image (zeros for an image no pair names).
inline std::vector<std::vector<double>> computeArrayDepthRectified(
    MultiEngine& m, const std::vector<ImageView>& raw, const std::vector<sva_rectify_view>& rect,
    const std::vector<Camera>& cameras, const std::vector<std::array<int, 2>>& pairs,
    const sva_sgm_params& p, int wmed_radius = 0, const std::array<uint16_t, 256>* weights = nullptr,
    int wmed_min_support = 1, bool wmed_select = false, int fill_max_dist = 0,
    int fill_min_found = 1, int fill_mode = SVA_FILL_SECOND, int speckle_max_size = 0,
    int speckle_max_diff = 0, int route = SVA_ARRAY_GROUPS, bool check = false, bool sub = false,
    int max_diff = 1, int min_agree = 1, int max_conflict = 0, int uniqueness = 0,
    int mode = SVA_FUSE_MEDIAN, double pitch = 0.05, int border = 0, bool mask = true,
    std::vector<std::vector<uint16_t>>* maps = nullptr,
    std::vector<std::vector<uint8_t>>* views = nullptr,
    std::vector<std::vector<uint8_t>>* valid = nullptr) {
    if (rect.size() != raw.size())
        throw Error(SVA_ERR_INVALID_ARG,
                    "computeArrayDepthRectified: need one sva_rectify_view per image");
    const detail::ChainFrame cf(raw, cameras, pairs, p, route, pitch, "computeArrayDepthRectified");
    const size_t np = (size_t)cf.fr.W * cf.fr.H, n = raw.size();
    std::vector<uint8_t> vw(views ? np * n : 0), vd(valid ? np * n : 0);
    auto depth = cf.depth(m, cameras, sva_array_depth_rectified, route, uniqueness, mode, maps, sub,
                          max_diff, min_agree, max_conflict, (uint8_t*)nullptr, (uint8_t*)nullptr,
                          check ? 1 : 0, speckle_max_size, speckle_max_diff, (uint32_t*)nullptr,
                          fill_max_dist, fill_min_found, fill_mode, (uint8_t*)nullptr, wmed_radius,
                          weights ? weights->data() : (const uint16_t*)nullptr, wmed_min_support,
                          wmed_select ? 1 : 0, (uint16_t*)nullptr, rect.data(), border,
                          mask ? 1 : 0, cf.ptr(vw), cf.ptr(vd));
    if (views) *views = detail::unpackPlanes(vw, np, n);
    if (valid) *valid = detail::unpackPlanes(vd, np, n);
    return depth;
}

// ---- refinement and 3-D output ----
// The reference's names and argument meaning; cv::Mat becomes ImageView (u8)
// or a dense W*H std::vector<double>.  Pixels a routine does not write keep
// the values of `init` (zeros when omitted) -- the reference leaves them
// uninitialised.

static_assert(sizeof(Point3d) == 3 * sizeof(double), "Point3d must be three packed doubles");

// shiftPerspectiveWithDisparity -- functions.cpp:55-77.
inline std::vector<uint8_t> shiftPerspectiveWithDisparity(Engine& eng, const Camera& inputCam,
                                                          const Camera& outputCam,
                                                          const ImageView& disparity,
                                                          const ImageView& image,
                                                          std::vector<uint8_t> init = {}) {
    if (disparity.width != image.width || disparity.height != image.height ||
        disparity.pitch != image.pitch)
        throw Error(SVA_ERR_INVALID_ARG, "shiftPerspectiveWithDisparity: plane mismatch");
    init.resize((size_t)image.height * image.pitch, 0);
    const sva_camera a = inputCam.abi(), b = outputCam.abi();
    eng.check(sva_shift_perspective(eng.handle(), &a, &b, disparity.data, image.data, image.width,
                                    image.height, image.pitch, init.data()));
    return init;
}

// improveWithDisparity -- functions.cpp:11-52.  `mask` replaces
// getFaceMask(centerImage) (:13; empty view = every pixel).  strict (default,
// as the reference): a masked pixel whose window leaves the image throws
// sva::Error, the analogue of the reference's cv::Exception on that ROI.
inline std::vector<uint8_t> improveWithDisparity(Engine& eng, const ImageView& disparity,
                                                 const ImageView& centerImage,
                                                 const std::vector<ImageView>& images,
                                                 const std::vector<std::array<Camera, 2>>& cameras,
                                                 int windowSize,
                                                 const ImageView& mask = ImageView(),
                                                 bool strict = true,
                                                 std::vector<uint8_t> init = {}) {
    const size_t pitch = centerImage.pitch;
    auto same = [&](const ImageView& v) {
        return v.width == centerImage.width && v.height == centerImage.height && v.pitch == pitch;
    };
    if (!same(disparity) || (mask.data && !same(mask)) || images.size() != cameras.size())
        throw Error(SVA_ERR_INVALID_ARG, "improveWithDisparity: plane or pair mismatch");
    std::vector<const uint8_t*> ptrs;
    std::vector<sva_camera> cams;
    for (size_t i = 0; i < images.size(); i++) {
        if (!same(images[i])) throw Error(SVA_ERR_INVALID_ARG, "improveWithDisparity: image size");
        ptrs.push_back(images[i].data);
        cams.push_back(cameras[i][0].abi());
        cams.push_back(cameras[i][1].abi());
    }
    init.resize((size_t)centerImage.height * pitch, 0);
    eng.check(sva_improve_with_disparity(eng.handle(), disparity.data, centerImage.data,
                                         ptrs.data(), cams.data(), (int)images.size(),
                                         centerImage.width, centerImage.height, pitch, mask.data,
                                         windowSize, strict ? 1 : 0, init.data()));
    return init;
}

// shiftPerspective2 -- functions.cpp:79-103 (depth map W*H f64).
inline std::vector<double> shiftPerspective2(Engine& eng, const Camera& inputCam,
                                             const Camera& outputCam,
                                             const std::vector<double>& depthMap, int W, int H,
                                             std::vector<double> init = {}) {
    if (depthMap.size() != (size_t)W * H) throw Error(SVA_ERR_INVALID_ARG, "depth map size");
    init.resize(depthMap.size(), 0.0);
    const sva_camera a = inputCam.abi(), b = outputCam.abi();
    eng.check(sva_shift_perspective2(eng.handle(), &a, &b, depthMap.data(), W, H, init.data()));
    return init;
}

// Points3DToDepthMap -- functions.cpp:118-132.
inline std::vector<double> Points3DToDepthMap(Engine& eng, const std::vector<Point3d>& points,
                                              const Camera& camera, int W, int H,
                                              std::vector<double> init = {}) {
    init.resize((size_t)W * H, 0.0);
    const sva_camera c = camera.abi();
    eng.check(sva_points_to_depth(eng.handle(), reinterpret_cast<const double*>(points.data()),
                                  (int64_t)points.size(), &c, W, H, init.data()));
    return init;
}

// DepthMapToPoints3D -- functions.cpp:134-146 (column-major order, depth > 0.1).
inline std::vector<Point3d> DepthMapToPoints3D(Engine& eng, const std::vector<double>& depthMap,
                                               const Camera& camera, int W, int H) {
    if (depthMap.size() != (size_t)W * H) throw Error(SVA_ERR_INVALID_ARG, "depth map size");
    std::vector<Point3d> pts((size_t)W * H);
    int64_t n = 0;
    const sva_camera c = camera.abi();
    eng.check(sva_depth_to_points(eng.handle(), depthMap.data(), W, H, &c,
                                  reinterpret_cast<double*>(pts.data()), &n));
    pts.resize((size_t)n);
    return pts;
}

// ---- ingestion ---------------------------------------

// getImagesPathsFromFolder -- functions.cpp:240-250, sorted by file name (the
// reference's directory_iterator order is unspecified).
inline std::vector<std::string> getImagesPathsFromFolder(const std::string& folderPath) {
    std::vector<std::string> filePaths;
    for (auto& p : std::filesystem::directory_iterator(folderPath))
        if (p.is_regular_file()) filePaths.push_back(p.path().u8string());
    std::sort(filePaths.begin(), filePaths.end());
    return filePaths;
}

// resize(img, img, Size(), 0.5, 0.5) -- CameraStereoVision.cpp:18 (INTER_LINEAR
// at exactly 2x = OpenCV's area path), on the GPU.  Returns a dense image of
// *outW x *outH.
inline std::vector<uint8_t> resizeHalf(Engine& eng, const ImageView& img, int* outW, int* outH) {
    int dw = 0, dh = 0;
    eng.check(sva_resize_half_size(img.width, img.height, &dw, &dh));
    std::vector<uint8_t> out((size_t)dw * dh);
    eng.check(sva_resize_half(eng.handle(), img.data, img.width, img.height, img.pitch,
                              out.data(), (size_t)(dw > 0 ? dw : 1)));
    if (outW) *outW = dw;
    if (outH) *outH = dh;
    return out;
}

// ---- evaluation ---------------------------------------

// A matrix of an OpenCV FileStorage "!!opencv-matrix" node: rows x cols x
// channels values of element code dt ('u' 'c' 'w' 's' 'i' 'f' 'd'), held as
// doubles (exact for every one of those types).
struct YamlMatrix {
    int rows = 0, cols = 0, channels = 1;
    char dt = 'd';
    std::vector<double> data;   // row-major, channels interleaved
};

namespace detail {
inline double yaml_number(const std::string& t) {
    if (t == ".Inf" || t == ".inf" || t == "+.Inf") return HUGE_VAL;
    if (t == "-.Inf" || t == "-.inf") return -HUGE_VAL;
    if (t == ".Nan" || t == ".nan" || t == ".NaN") return std::nan("");
    size_t used = 0;
    const double v = std::stod(t, &used);
    if (used != t.size()) throw Error(SVA_ERR_INVALID_ARG, "yaml: bad number '" + t + "'");
    return v;
}
inline std::string yaml_field(const std::string& body, const std::string& name) {
    std::istringstream in(body);
    std::string line;
    while (std::getline(in, line)) {
        const size_t a = line.find_first_not_of(" \t");
        if (a == std::string::npos || a == 0) continue;   // nested fields are indented
        if (line.compare(a, name.size() + 1, name + ":") == 0) {
            std::string v = line.substr(a + name.size() + 1);
            v.erase(0, v.find_first_not_of(" \t\""));
            v.erase(v.find_last_not_of(" \t\"\r") + 1);
            return v;
        }
    }
    throw Error(SVA_ERR_INVALID_ARG, "yaml: missing field " + name);
}
}  // namespace detail

// FileStorage(path, READ)[key] >> Mat for an "!!opencv-matrix" node.
inline YamlMatrix readYamlMatrix(const std::string& path, const std::string& key) {
    std::ifstream f(path);
    if (!f) throw Error(SVA_ERR_INVALID_ARG, "cannot open " + path);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    const std::string head = key + ":";
    size_t pos = 0, start = std::string::npos;
    while ((pos = text.find(head, pos)) != std::string::npos) {
        const bool bol = pos == 0 || text[pos - 1] == '\n';
        const size_t eol = text.find('\n', pos);
        const std::string rest = text.substr(pos + head.size(), eol - pos - head.size());
        if (bol && rest.find("!!opencv-matrix") != std::string::npos) {
            start = eol;
            break;
        }
        pos += head.size();
    }
    if (start == std::string::npos) throw Error(SVA_ERR_INVALID_ARG, "yaml: no matrix " + key);
    // the node ends at the next unindented line
    size_t end = start;
    while (end < text.size()) {
        const size_t nl = text.find('\n', end + 1);
        const size_t ls = end + 1;
        if (ls < text.size() && text[ls] != ' ' && text[ls] != '\t' && text[ls] != '\n') break;
        if (nl == std::string::npos) { end = text.size(); break; }
        end = nl;
    }
    const std::string body = text.substr(start, end - start);
    YamlMatrix m;
    m.rows = std::stoi(detail::yaml_field(body, "rows"));
    m.cols = std::stoi(detail::yaml_field(body, "cols"));
    const std::string dt = detail::yaml_field(body, "dt");
    if (dt.empty() || std::string("ucwsifd").find(dt.back()) == std::string::npos)
        throw Error(SVA_ERR_INVALID_ARG, "yaml: unsupported dt " + dt);
    m.dt = dt.back();
    m.channels = dt.size() > 1 ? std::stoi(dt.substr(0, dt.size() - 1)) : 1;
    const size_t lb = body.find('['), rb = body.find(']', lb);
    if (lb == std::string::npos || rb == std::string::npos)
        throw Error(SVA_ERR_INVALID_ARG, "yaml: missing data");
    std::string tok;
    for (size_t i = lb + 1; i <= rb; i++) {
        const char ch = body[i];
        if (ch == ',' || ch == ']' || ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r') {
            if (!tok.empty()) m.data.push_back(detail::yaml_number(tok));
            tok.clear();
        } else {
            tok += ch;
        }
    }
    if (m.data.size() != (size_t)m.rows * m.cols * m.channels)
        throw Error(SVA_ERR_INVALID_ARG, "yaml: data size does not match rows x cols");
    return m;
}

// FileStorage(path, WRITE) << key << Mat (a new file holding one node).
inline void writeYamlMatrix(const std::string& path, const std::string& key, const YamlMatrix& m) {
    if (m.data.size() != (size_t)m.rows * m.cols * m.channels)
        throw Error(SVA_ERR_INVALID_ARG, "yaml: data size does not match rows x cols");
    std::ofstream f(path);
    if (!f) throw Error(SVA_ERR_INVALID_ARG, "cannot write " + path);
    f << "%YAML:1.0\n---\n" << key << ": !!opencv-matrix\n   rows: " << m.rows
      << "\n   cols: " << m.cols << "\n   dt: ";
    if (m.channels > 1) f << m.channels;
    f << m.dt << "\n   data: [ ";
    const bool fl = m.dt == 'f' || m.dt == 'd';
    char buf[64];
    for (size_t i = 0; i < m.data.size(); i++) {
        const double v = m.data[i];
        if (fl && std::isnan(v)) std::snprintf(buf, sizeof buf, ".Nan");
        else if (fl && std::isinf(v)) std::snprintf(buf, sizeof buf, v > 0 ? ".Inf" : "-.Inf");
        else if (fl) std::snprintf(buf, sizeof buf, m.dt == 'f' ? "%.9g" : "%.17g", v);
        else std::snprintf(buf, sizeof buf, "%lld", (long long)v);
        f << buf << (i + 1 < m.data.size() ? ((i + 1) % 8 ? ", " : ",\n       ") : "");
    }
    f << " ]\n";
}

// getIdealRef -- functions.cpp:323-329 ("idealRef.yml", key "R").
inline YamlMatrix getIdealRef(const std::string& path = "idealRef.yml") {
    return readYamlMatrix(path, "R");
}
// saveImage / loadImage -- functions.cpp:331-346 (key "image").
inline void saveImage(const std::string& filename, const YamlMatrix& image) {
    writeYamlMatrix(filename, "image", image);
}
inline YamlMatrix loadImage(const std::string& filename) { return readYamlMatrix(filename, "image"); }

// resize(src, dst, Size(dw, dh)) INTER_LINEAR on a dense f64 matrix, on the GPU.
inline std::vector<double> resizeLinear(Engine& eng, const std::vector<double>& src, int sw, int sh,
                                        int dw, int dh) {
    if (src.size() != (size_t)sw * sh) throw Error(SVA_ERR_INVALID_ARG, "resize: size mismatch");
    std::vector<double> out((size_t)dw * dh);
    eng.check(sva_resize_linear_f64(eng.handle(), src.data(), sw, sh, out.data(), dw, dh));
    return out;
}

// CameraStereoVision.cpp:107-110,118-119: resize(depth, depth2, ref.size());
// error = (depth2 - ref) * scale -- on the GPU, returned at ref's size.
inline std::vector<double> refError(Engine& eng, const std::vector<double>& depth, int w, int h,
                                    const YamlMatrix& ref, double scale = 50.0) {
    if (depth.size() != (size_t)w * h || ref.channels != 1 ||
        ref.data.size() != (size_t)ref.rows * ref.cols)
        throw Error(SVA_ERR_INVALID_ARG, "refError: size mismatch");
    std::vector<double> err(ref.data.size());
    eng.check(sva_ref_error(eng.handle(), depth.data(), w, h, ref.data.data(), ref.cols, ref.rows,
                            scale, err.data()));
    return err;
}

// calculateAverageError -- functions.cpp:348-354: cv::mean(image, mask)[0] on
// the GPU.  mask (W*H, nullable = all) replaces dlib's getFaceMask.
inline double calculateAverageError(Engine& eng, const std::vector<double>& image, int w, int h,
                                    const std::vector<uint8_t>* mask = nullptr) {
    if (image.size() != (size_t)w * h || (mask && mask->size() != image.size()))
        throw Error(SVA_ERR_INVALID_ARG, "calculateAverageError: size mismatch");
    double mean = 0;
    eng.check(sva_masked_mean(eng.handle(), image.data(), mask ? mask->data() : nullptr, w, h,
                              &mean));
    return mean;
}

}  // namespace sva
