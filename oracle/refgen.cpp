// refgen -- runs the reference's own Camera.cpp, functions.cpp and
// CameraStereoVision.cpp (compiled unmodified against oracle/cvstandin) on
// inputs that tests/golden/make_ref_golden.py writes, and dumps what they
// compute.  TEST INFRASTRUCTURE ONLY; the binary lands in oracle/_ref/ and is
// never committed.
//
//   refgen <case> <indir> <outdir> <fill> [ints...]
//
// <fill> is the byte that new Mat{size, type} storage holds (the reference
// leaves it uninitialised); the maker runs every case with 0x00 and 0xA5 and
// records where the two outputs agree.  Arrays travel as files "<name>.bin":
// one text line "<u8|i32|f64> <ndim> <dims...>\n", then the raw little-endian
// data.  Nothing here restates a reference loop: the hot loop only ever runs
// as reference_main(), and every other case is one call of a reference
// function per input.
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include <unistd.h>

#include "Camera.h"
#include "functions.h"
#include "dlibFaceSelect.h"

#undef main
int reference_main();

namespace {

cv::Mat g_face_mask;
std::string g_in, g_out;

[[noreturn]] void die(const std::string& why) {
    std::fprintf(stderr, "refgen: %s\n", why.c_str());
    std::exit(2);
}

struct Blob {
    std::string dtype;
    std::vector<long> dims;
    std::vector<uint8_t> data;
    long count() const {
        long n = 1;
        for (long d : dims) n *= d;
        return n;
    }
    template <typename T> const T* as() const { return reinterpret_cast<const T*>(data.data()); }
};

size_t width_of(const std::string& dt) {
    if (dt == "u8") return 1;
    if (dt == "i32") return 4;
    if (dt == "f64") return 8;
    die("unknown dtype " + dt);
}

Blob load(const std::string& name) {
    std::ifstream f(g_in + "/" + name + ".bin", std::ios::binary);
    if (!f) die("cannot read input " + name);
    std::string line;
    std::getline(f, line);
    std::istringstream hs(line);
    Blob b;
    int nd = 0;
    hs >> b.dtype >> nd;
    for (int i = 0; i < nd; i++) {
        long d = 0;
        hs >> d;
        b.dims.push_back(d);
    }
    if (!hs) die("bad header in " + name);
    b.data.resize((size_t)b.count() * width_of(b.dtype));
    f.read(reinterpret_cast<char*>(b.data.data()), (std::streamsize)b.data.size());
    if ((size_t)f.gcount() != b.data.size()) die("short input " + name);
    return b;
}

void save(const std::string& name, const std::string& dt, const std::vector<long>& dims,
          const void* data) {
    std::ofstream f(g_out + "/" + name + ".bin", std::ios::binary);
    long n = 1;
    f << dt << " " << dims.size();
    for (long d : dims) {
        f << " " << d;
        n *= d;
    }
    f << "\n";
    f.write(reinterpret_cast<const char*>(data), (std::streamsize)((size_t)n * width_of(dt)));
    if (!f) die("cannot write output " + name);
}

// 2-D plane <-> Mat.  Copies, so a Mat never aliases a Blob.
cv::Mat to_mat(const Blob& b, long plane = 0) {
    const size_t nd = b.dims.size();
    if (nd < 2) die("plane expected");
    const int H = (int)b.dims[nd - 2], W = (int)b.dims[nd - 1];
    const int type = b.dtype == "u8" ? CV_8U : b.dtype == "f64" ? CV_64F : -1;
    if (type < 0) die("u8 or f64 plane expected");
    const size_t es = width_of(b.dtype);
    cv::Mat m(H, W, type);
    for (int y = 0; y < H; y++)
        std::memcpy(m.ptr(y), b.data.data() + ((size_t)plane * H + y) * W * es, (size_t)W * es);
    return m;
}

void save_mat(const std::string& name, const cv::Mat& m) {
    if (m.empty()) die("nothing to save for " + name);
    const size_t es = cv::elemSizeOf(m.type());
    std::vector<uint8_t> flat((size_t)m.rows * m.cols * es);
    for (int y = 0; y < m.rows; y++)
        std::memcpy(flat.data() + (size_t)y * m.cols * es, m.ptr(y), (size_t)m.cols * es);
    save(name, m.type() == CV_8U ? "u8" : m.type() == CV_64F ? "f64" : "f32?", {m.rows, m.cols},
         flat.data());
}

// cams.bin: f64 [n][5] = f, x, y, z, pixel_size
std::vector<Camera> load_cameras() {
    Blob b = load("cams");
    if (b.dtype != "f64" || b.dims.size() != 2 || b.dims[1] != 5) die("cams: f64 [n][5] expected");
    std::vector<Camera> cams;
    for (long i = 0; i < b.dims[0]; i++) {
        const double* c = b.as<double>() + 5 * i;
        cams.emplace_back(c[0], cv::Point3d{c[1], c[2], c[3]}, c[4]);
    }
    return cams;
}

const cv::Mat& shown(const std::string& name) {
    auto& s = cv::standin::state().shown;
    auto it = s.find(name);
    if (it == s.end()) die("the reference never showed \"" + name + "\"");
    return it->second;
}

int arg_int(const std::vector<std::string>& a, size_t i) {
    if (i >= a.size()) die("missing integer argument");
    return std::atoi(a[i].c_str());
}

// ---- cases -------------------------------------------------------------------

// The unmodified main(): 25 views through imread, the mask through
// getFaceMask, a zero idealRef; outputs picked up from what it shows.  It
// looks for its images in ./Renders2, so it runs in a scratch directory with
// 25 empty placeholder files there.
void case_main() {
    Blob views = load("views");
    if (views.dtype != "u8" || views.dims.size() != 3 || views.dims[0] != 25) die("views: u8 [25][H][W]");
    auto& st = cv::standin::state();
    for (long i = 0; i < 25; i++) st.images.push_back(to_mat(views, i));
    g_face_mask = to_mat(load("mask"));
    cv::Mat ref(g_face_mask.rows, g_face_mask.cols, CV_64F);
    for (int y = 0; y < ref.rows; y++)
        for (int x = 0; x < ref.cols; x++) ref.at<double>(y, x) = 0.0;
    st.stored["R"] = ref;

    namespace fs = std::filesystem;
    const fs::path out_abs = fs::absolute(g_out);
    g_out = out_abs.string();
    const fs::path work = out_abs / "cwd";
    fs::create_directories(work / "Renders2");
    for (int i = 0; i < 25; i++) {
        char name[32];
        std::snprintf(name, sizeof name, "%02d.png", i);
        std::ofstream(work / "Renders2" / name);
    }
    if (chdir(work.c_str()) != 0) die("chdir failed");
    // The last statements of main() subtract an f64 Mat from a u8 one, which
    // the library rejects and the stand-in rejects too: main() ends there by
    // exception, after everything recorded below has been shown.
    bool ended_by_exception = false;
    try {
        reference_main();
    } catch (const cv::Exception&) {
        ended_by_exception = true;
    }
    if (!ended_by_exception) die("main() was expected to end at its mixed-type subtraction");
    if (st.imread_calls != 25) die("main() did not read 25 images");
    save_mat("disparity", shown("Disparity"));
    save_mat("depth", shown("Depth"));
    save_mat("improved", shown("Depth2"));
    fs::remove_all(work);
}

void case_bresenham() {
    Blob p = load("pairs");
    if (p.dtype != "i32" || p.dims.size() != 2 || p.dims[1] != 4) die("pairs: i32 [n][4]");
    std::vector<int32_t> pts, offsets{0};
    for (long i = 0; i < p.dims[0]; i++) {
        const int32_t* q = p.as<int32_t>() + 4 * i;
        for (const cv::Point2i& pt : bresenham(cv::Point2i(q[0], q[1]), cv::Point2i(q[2], q[3]))) {
            pts.push_back(pt.x);
            pts.push_back(pt.y);
        }
        offsets.push_back((int32_t)(pts.size() / 2));
    }
    save("points", "i32", {(long)pts.size() / 2, 2}, pts.data());
    save("offsets", "i32", {(long)offsets.size()}, offsets.data());
}

void case_camera() {
    std::vector<Camera> cams = load_cameras();
    Blob pix = load("pixels"), pts = load("points");
    if (pix.dtype != "i32" || pts.dtype != "f64") die("pixels: i32 [n][2], points: f64 [n][3]");
    const long np = pix.dims[0], nq = pts.dims[0];
    std::vector<int32_t> proj;
    std::vector<double> inv;
    for (Camera& c : cams) {
        for (long i = 0; i < nq; i++) {
            const double* q = pts.as<double>() + 3 * i;
            cv::Point2i r = c.project(cv::Point3d{q[0], q[1], q[2]});
            proj.push_back(r.x);
            proj.push_back(r.y);
        }
        for (long i = 0; i < np; i++) {
            const int32_t* q = pix.as<int32_t>() + 2 * i;
            cv::Point3d r = c.inv_project(cv::Point2i(q[0], q[1]));
            inv.push_back(r.x);
            inv.push_back(r.y);
            inv.push_back(r.z);
        }
    }
    save("project", "i32", {(long)cams.size(), nq, 2}, proj.data());
    save("inv_project", "f64", {(long)cams.size(), np, 3}, inv.data());
}

void json_pairs(std::ostream& o, const std::vector<std::array<int, 2>>& v) {
    o << "[";
    for (size_t i = 0; i < v.size(); i++) o << (i ? ", " : "") << "[" << v[i][0] << ", " << v[i][1] << "]";
    o << "]";
}

// Every pairType (numbered as the enum is) through both overloads, and CHESS.
void case_pairs() {
    std::vector<Camera> cams = load_cameras();
    std::ofstream o(g_out + "/pairs.json");
    o << "[\n";
    for (int t = ORTHOGONAL; t <= MID_TOP; t++) {
        o << " {\"call\": \"getCameraPairs\", \"pairType\": " << t << ", \"pairs\": ";
        json_pairs(o, getCameraPairs(cams, (pairType)t));
        o << "},\n";
    }
    for (int t = ORTHOGONAL; t <= MID_TOP; t++)
        for (int n = 0; n < 25; n++) {
            o << " {\"call\": \"getCameraPairs\", \"pairType\": " << t << ", \"cameraNum\": " << n
              << ", \"pairs\": ";
            json_pairs(o, getCameraPairs(cams, (pairType)t, n));
            o << "},\n";
        }
    o << " {\"call\": \"getGroups\", \"groupType\": \"CHESS\", \"groups\": [";
    auto groups = getGroups(cams, "CHESS");
    for (size_t i = 0; i < groups.size(); i++) {
        o << (i ? ", " : "");
        json_pairs(o, groups[i]);
    }
    o << "]}\n]\n";
}

// shiftPerspectiveWithDisparity(cams[a], cams[b], disp, image)
void case_shift(const std::vector<std::string>& a) {
    std::vector<Camera> cams = load_cameras();
    cv::Mat disp = to_mat(load("disp")), img = to_mat(load("image"));
    save_mat("shifted", shiftPerspectiveWithDisparity(cams.at(arg_int(a, 0)), cams.at(arg_int(a, 1)), disp, img));
}

// improveWithDisparity(disp, center, {image}, {{cams[a], cams[b]}}, window)
void case_improve(const std::vector<std::string>& a) {
    std::vector<Camera> cams = load_cameras();
    cv::Mat disp = to_mat(load("disp")), center = to_mat(load("center"));
    std::vector<cv::Mat> images{to_mat(load("image"))};
    g_face_mask = to_mat(load("mask"));
    std::vector<std::array<Camera, 2>> pairs{{cams.at(arg_int(a, 0)), cams.at(arg_int(a, 1))}};
    int32_t threw = 0;
    cv::Mat out;
    try {
        out = improveWithDisparity(disp, center, images, pairs, arg_int(a, 2));
    } catch (const cv::Exception&) {
        threw = 1;
    }
    save("threw", "i32", {1}, &threw);
    if (!threw) save_mat("improved", out);
}

// shiftPerspective2(cams[a], cams[b], depth)
void case_shift2(const std::vector<std::string>& a) {
    std::vector<Camera> cams = load_cameras();
    cv::Mat depth = to_mat(load("depth"));
    save_mat("shifted", shiftPerspective2(cams.at(arg_int(a, 0)), cams.at(arg_int(a, 1)), depth));
}

// Points3DToDepthMap(points, cams[a], Size(W, H))
void case_points_to_depth(const std::vector<std::string>& a) {
    std::vector<Camera> cams = load_cameras();
    Blob p = load("points");
    if (p.dtype != "f64" || p.dims.size() != 2 || p.dims[1] != 3) die("points: f64 [n][3]");
    std::vector<cv::Point3d> pts;
    for (long i = 0; i < p.dims[0]; i++) {
        const double* q = p.as<double>() + 3 * i;
        pts.emplace_back(q[0], q[1], q[2]);
    }
    save_mat("depth", Points3DToDepthMap(pts, cams.at(arg_int(a, 0)), cv::Size(arg_int(a, 1), arg_int(a, 2))));
}

// DepthMapToPoints3D(depth, cams[a], depth.size())
void case_depth_to_points(const std::vector<std::string>& a) {
    std::vector<Camera> cams = load_cameras();
    cv::Mat depth = to_mat(load("depth"));
    std::vector<cv::Point3d> pts = DepthMapToPoints3D(depth, cams.at(arg_int(a, 0)), depth.size());
    std::vector<double> flat;
    for (const cv::Point3d& p : pts) {
        flat.push_back(p.x);
        flat.push_back(p.y);
        flat.push_back(p.z);
    }
    save("points", "f64", {(long)pts.size(), 3}, flat.data());
}

}  // namespace

// Link stubs for dlibFaceSelect.cpp (dlib is not part of this build): the mask
// is whatever the case set.
cv::Mat getFaceMask(cv::Mat&) { return g_face_mask.clone(); }
cv::Mat getFaceCircle(cv::Mat& image) { return image; }

int main(int argc, char** argv) {
    if (argc < 5) die("usage: refgen <case> <indir> <outdir> <fill> [ints...]");
    const std::string name = argv[1];
    g_in = std::filesystem::absolute(argv[2]).string();
    g_out = std::filesystem::absolute(argv[3]).string();
    const std::vector<std::string> rest(argv + 5, argv + argc);
    // input Mats are overwritten whole after they are made, so the fill byte
    // survives only in storage the reference allocates and leaves unwritten
    cv::standin::state().fill_byte = (uint8_t)std::strtol(argv[4], nullptr, 0);

    std::ostringstream chatter;                 // the reference prints as it goes
    std::streambuf* saved = std::cout.rdbuf(chatter.rdbuf());

    if (name == "main") case_main();
    else if (name == "bresenham") case_bresenham();
    else if (name == "camera") case_camera();
    else if (name == "pairs") case_pairs();
    else if (name == "shift") case_shift(rest);
    else if (name == "improve") case_improve(rest);
    else if (name == "shift2") case_shift2(rest);
    else if (name == "points_to_depth") case_points_to_depth(rest);
    else if (name == "depth_to_points") case_depth_to_points(rest);
    else die("unknown case " + name);
    std::cout.rdbuf(saved);
    return 0;
}
