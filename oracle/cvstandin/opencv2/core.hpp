// Stand-in for the slice of <opencv2/core.hpp> that the reference's
// Camera.cpp, functions.cpp and CameraStereoVision.cpp use.  TEST
// INFRASTRUCTURE ONLY: it exists so that oracle/refgen.cpp can run those three
// files unmodified and record what they compute (oracle/Makefile, target ref).
//
// This is not OpenCV and shares no text with it.  Integer paths, loop order and
// truncations are the reference's own code; what this file restates is the
// library arithmetic the reference calls (absdiff + sum, multiply, scalar /
// Mat, norm, cvRound, resize, mean), written from the documented behaviour.
//
// Differences from the library that the driver relies on:
//   * Mat{size, type} storage is filled with cv::standin::state().fill_byte
//     (the library leaves it uninitialised);
//   * imread, imshow, FileStorage and the window calls route to hooks in
//     cv::standin::state() instead of touching files or a display.
#ifndef SVA_CVSTANDIN_CORE_HPP
#define SVA_CVSTANDIN_CORE_HPP

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5
#define CV_64F 6
#define CV_8UC1 0
#define CV_32FC1 5
#define CV_64FC1 6

namespace cv {

class Exception : public std::runtime_error {
public:
    explicit Exception(const std::string& what) : std::runtime_error(what) {}
};

// Round half to even, as the library's cvRound does on its default path.
inline int cvRound(double v) { return (int)std::nearbyint(v); }

template <typename T> struct Size_;

template <typename T> struct Point_ {
    T x{}, y{};
    Point_() = default;
    Point_(T x_, T y_) : x(x_), y(y_) {}
    Point_(const Size_<T>& s);
    // Point2d -> Point2i and the like: integers round, they do not truncate.
    template <typename U> explicit operator Point_<U>() const {
        if constexpr (std::is_integral<U>::value && std::is_floating_point<T>::value)
            return Point_<U>((U)cvRound((double)x), (U)cvRound((double)y));
        else
            return Point_<U>((U)x, (U)y);
    }
};
typedef Point_<int> Point2i;
typedef Point_<double> Point2d;
typedef Point2i Point;

template <typename T> Point_<T> operator+(const Point_<T>& a, const Point_<T>& b) { return {T(a.x + b.x), T(a.y + b.y)}; }
template <typename T> Point_<T> operator-(const Point_<T>& a, const Point_<T>& b) { return {T(a.x - b.x), T(a.y - b.y)}; }
template <typename T> Point_<T> operator*(const Point_<T>& a, int s) { return {T(a.x * s), T(a.y * s)}; }
template <typename T> Point_<T> operator*(const Point_<T>& a, double s) {
    if constexpr (std::is_integral<T>::value) return {(T)cvRound(a.x * s), (T)cvRound(a.y * s)};
    else return {T(a.x * s), T(a.y * s)};
}
template <typename T> bool operator==(const Point_<T>& a, const Point_<T>& b) { return a.x == b.x && a.y == b.y; }
template <typename T> std::ostream& operator<<(std::ostream& o, const Point_<T>& p) { return o << "[" << p.x << ", " << p.y << "]"; }

template <typename T> struct Point3_ {
    T x{}, y{}, z{};
    Point3_() = default;
    Point3_(T x_, T y_, T z_) : x(x_), y(y_), z(z_) {}
};
typedef Point3_<double> Point3d;
template <typename T> Point3_<T> operator+(const Point3_<T>& a, const Point3_<T>& b) { return {T(a.x + b.x), T(a.y + b.y), T(a.z + b.z)}; }
template <typename T> Point3_<T> operator-(const Point3_<T>& a, const Point3_<T>& b) { return {T(a.x - b.x), T(a.y - b.y), T(a.z - b.z)}; }
template <typename T> Point3_<T> operator*(const Point3_<T>& a, double s) { return {T(a.x * s), T(a.y * s), T(a.z * s)}; }
template <typename T> Point3_<T> operator/(const Point3_<T>& a, double s) { return {T(a.x / s), T(a.y / s), T(a.z / s)}; }
template <typename T> std::ostream& operator<<(std::ostream& o, const Point3_<T>& p) { return o << "[" << p.x << ", " << p.y << ", " << p.z << "]"; }

template <typename T> struct Size_ {
    T width{}, height{};
    Size_() = default;
    Size_(T w, T h) : width(w), height(h) {}
};
typedef Size_<int> Size;
template <typename T> Point_<T>::Point_(const Size_<T>& s) : x(s.width), y(s.height) {}
template <typename T> Size_<T> operator/(const Size_<T>& a, T s) { return {T(a.width / s), T(a.height / s)}; }
template <typename T> bool operator==(const Size_<T>& a, const Size_<T>& b) { return a.width == b.width && a.height == b.height; }
template <typename T> std::ostream& operator<<(std::ostream& o, const Size_<T>& s) { return o << "[" << s.width << " x " << s.height << "]"; }

struct Rect {
    int x = 0, y = 0, width = 0, height = 0;
    Rect() = default;
    Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
    // Two corners: top-left inclusive, bottom-right exclusive.
    Rect(const Point2i& a, const Point2i& b)
        : x(std::min(a.x, b.x)), y(std::min(a.y, b.y)),
          width(std::max(a.x, b.x) - std::min(a.x, b.x)),
          height(std::max(a.y, b.y) - std::min(a.y, b.y)) {}
};

struct Scalar {
    double val[4] = {0, 0, 0, 0};
    Scalar() = default;
    Scalar(double v0) { val[0] = v0; }
    double& operator[](int i) { return val[i]; }
    const double& operator[](int i) const { return val[i]; }
};

inline double norm(double v) { return std::fabs(v); }
template <typename T> double norm(const Point_<T>& p) { return std::sqrt((double)p.x * p.x + (double)p.y * p.y); }
template <typename T> double norm(const Point3_<T>& p) {
    return std::sqrt((double)p.x * p.x + (double)p.y * p.y + (double)p.z * p.z);
}

class Mat;
namespace standin {
struct State;
State& state();
}  // namespace standin

inline size_t elemSizeOf(int type) {
    switch (type) {
        case CV_8U: return 1;
        case CV_32F: return 4;
        case CV_64F: return 8;
    }
    throw Exception("stand-in Mat: unsupported type");
}

// Single-channel matrix; copies share storage, operator()(Rect) is a view.
class Mat {
public:
    int rows = 0, cols = 0;

    Mat() = default;
    Mat(Size s, int type) { create(s.height, s.width, type); }
    Mat(int r, int c, int type) { create(r, c, type); }
    template <typename T> explicit Mat(std::initializer_list<T> l) {
        static_assert(std::is_same<T, int>::value, "stand-in Mat: int lists only");
        create((int)l.size(), 1, CV_8U);
    }

    void create(int r, int c, int type);   // new storage, filled with the fill byte
    int type() const { return type_; }
    Size size() const { return Size(cols, rows); }
    bool empty() const { return !buf_ || rows == 0 || cols == 0; }
    size_t step() const { return step_; }
    uint8_t* ptr(int y) { return base_ + (size_t)y * step_; }
    const uint8_t* ptr(int y) const { return base_ + (size_t)y * step_; }

    template <typename T> T& at(int y, int x) { return reinterpret_cast<T*>(ptr(y))[x]; }
    template <typename T> const T& at(int y, int x) const { return reinterpret_cast<const T*>(ptr(y))[x]; }
    template <typename T> T& at(Point p) { return at<T>(p.y, p.x); }
    template <typename T> const T& at(Point p) const { return at<T>(p.y, p.x); }

    Mat operator()(const Rect& r) const {
        if (r.x < 0 || r.y < 0 || r.width < 0 || r.height < 0 || r.x + r.width > cols ||
            r.y + r.height > rows)
            throw Exception("stand-in Mat: ROI leaves the image");
        Mat v(*this);
        v.rows = r.height;
        v.cols = r.width;
        v.base_ = base_ + (size_t)r.y * step_ + (size_t)r.x * elemSizeOf(type_);
        return v;
    }

    Mat clone() const {
        Mat m;
        if (!buf_) return m;
        m.create(rows, cols, type_);
        for (int y = 0; y < rows; y++) std::memcpy(m.ptr(y), ptr(y), (size_t)cols * elemSizeOf(type_));
        return m;
    }

    // Element as f64, whatever the type.
    double get(int y, int x) const {
        switch (type_) {
            case CV_8U: return at<uint8_t>(y, x);
            case CV_32F: return at<float>(y, x);
            default: return at<double>(y, x);
        }
    }

private:
    int type_ = CV_8U;
    size_t step_ = 0;
    std::shared_ptr<std::vector<uint8_t>> buf_;
    uint8_t* base_ = nullptr;
};

// Lazy A - B, |A - B|, (A - B) * s and s / A; evaluated on conversion to Mat.
class MatExpr {
public:
    enum Kind { SUB, ABSDIFF, RDIV };
    Kind kind;
    Mat a, b;
    double s = 1.0;
    operator Mat() const;
};

inline MatExpr operator-(const Mat& a, const Mat& b) { return MatExpr{MatExpr::SUB, a, b, 1.0}; }
inline MatExpr operator/(double s, const Mat& a) { return MatExpr{MatExpr::RDIV, a, Mat(), s}; }
inline MatExpr operator*(const MatExpr& e, double s) {
    if (e.kind == MatExpr::RDIV) throw Exception("stand-in MatExpr: unsupported product");
    MatExpr r = e;
    r.s = e.s * s;
    return r;
}
inline MatExpr abs(const MatExpr& e) {
    if (e.kind != MatExpr::SUB || e.s != 1.0) throw Exception("stand-in MatExpr: unsupported abs");
    MatExpr r = e;
    r.kind = MatExpr::ABSDIFF;
    return r;
}

Scalar sum(const Mat& m);
Scalar mean(const Mat& m, const Mat& mask = Mat());
void multiply(const Mat& a, double s, Mat& dst, double scale = 1.0, int dtype = -1);

// ---- files: every read and write goes to the driver's hooks ----------------
class FileNode {
public:
    std::string key;
};
void operator>>(const FileNode& n, Mat& m);

class FileStorage {
public:
    enum Mode { READ = 0, WRITE = 1 };
    FileStorage() = default;
    FileStorage(const std::string& name, int mode) { open(name, mode); }
    bool open(const std::string& name, int mode) {
        name_ = name;
        mode_ = mode;
        return true;
    }
    FileNode operator[](const char* key) const { return FileNode{key}; }
    FileStorage& operator<<(const char* key) {
        pending_ = key;
        return *this;
    }
    FileStorage& operator<<(const Mat& m);

private:
    std::string name_, pending_;
    int mode_ = READ;
};

namespace standin {
struct State {
    uint8_t fill_byte = 0;                       // content of new Mat storage
    int imread_calls = 0;                        // imread returns images[imread_calls++]
    std::vector<Mat> images;
    std::map<std::string, Mat> shown;            // imshow(name, m): last copy per name
    std::map<std::string, Mat> stored;           // FileStorage reads (by key) and writes
};
inline State& state() {
    static State s;
    return s;
}
}  // namespace standin

inline void Mat::create(int r, int c, int type) {
    if (r < 0 || c < 0) throw Exception("stand-in Mat: negative size");
    rows = r;
    cols = c;
    type_ = type;
    step_ = (size_t)c * elemSizeOf(type);
    buf_ = std::make_shared<std::vector<uint8_t>>((size_t)r * step_ + 1, standin::state().fill_byte);
    base_ = buf_->data();
}

inline MatExpr::operator Mat() const {
    Mat out;
    if (kind == RDIV) {                          // s / A, 0 where A is 0
        if (a.type() != CV_64F) throw Exception("stand-in MatExpr: s / A needs f64");
        out.create(a.rows, a.cols, CV_64F);
        for (int y = 0; y < a.rows; y++)
            for (int x = 0; x < a.cols; x++) {
                double d = a.at<double>(y, x);
                out.at<double>(y, x) = d != 0.0 ? s / d : 0.0;
            }
        return out;
    }
    if (a.type() != b.type()) throw Exception("stand-in MatExpr: operand types differ");
    if (a.rows != b.rows || a.cols != b.cols) throw Exception("stand-in MatExpr: operand sizes differ");
    out.create(a.rows, a.cols, a.type());
    for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < a.cols; x++) {
            if (a.type() == CV_8U) {
                int d = (int)a.at<uint8_t>(y, x) - (int)b.at<uint8_t>(y, x);
                if (kind == ABSDIFF) d = d < 0 ? -d : d;
                double v = s == 1.0 ? (double)d : d * s;
                int r = s == 1.0 ? d : cvRound(v);
                out.at<uint8_t>(y, x) = (uint8_t)std::min(255, std::max(0, r));
            } else if (a.type() == CV_64F) {
                double d = a.at<double>(y, x) - b.at<double>(y, x);
                if (kind == ABSDIFF) d = std::fabs(d);
                out.at<double>(y, x) = s == 1.0 ? d : d * s;
            } else {
                float d = a.at<float>(y, x) - b.at<float>(y, x);
                if (kind == ABSDIFF) d = std::fabs(d);
                out.at<float>(y, x) = s == 1.0 ? d : (float)(d * s);
            }
        }
    return out;
}

inline Scalar sum(const Mat& m) {               // f64 accumulator, row-major
    double acc = 0.0;
    for (int y = 0; y < m.rows; y++)
        for (int x = 0; x < m.cols; x++) acc += m.get(y, x);
    return Scalar(acc);
}

inline Scalar mean(const Mat& m, const Mat& mask) {
    double acc = 0.0;
    long long n = 0;
    for (int y = 0; y < m.rows; y++)
        for (int x = 0; x < m.cols; x++) {
            if (!mask.empty() && mask.at<uint8_t>(y, x) == 0) continue;
            acc += m.get(y, x);
            n++;
        }
    return Scalar(n ? acc / (double)n : 0.0);
}

inline void multiply(const Mat& a, double s, Mat& dst, double scale, int dtype) {
    if (dtype != CV_64F) throw Exception("stand-in multiply: f64 output only");
    Mat out(a.rows, a.cols, CV_64F);
    for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < a.cols; x++)
            out.at<double>(y, x) = scale == 1.0 ? a.get(y, x) * s : a.get(y, x) * s * scale;
    dst = out;
}

inline void operator>>(const FileNode& n, Mat& m) {
    auto& st = standin::state().stored;
    auto it = st.find(n.key);
    m = it == st.end() ? Mat() : it->second.clone();
}

inline FileStorage& FileStorage::operator<<(const Mat& m) {
    standin::state().stored[pending_] = m.clone();
    return *this;
}

}  // namespace cv
#endif
