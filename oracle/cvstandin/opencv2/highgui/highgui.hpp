// Stand-in for <opencv2/highgui/highgui.hpp>: no files, no windows.  imread
// hands out the driver's images in call order and imshow records what it is
// shown (see core.hpp in this folder).
#ifndef SVA_CVSTANDIN_HIGHGUI_HPP
#define SVA_CVSTANDIN_HIGHGUI_HPP

#include "../core.hpp"

namespace cv {

enum { IMREAD_GRAYSCALE = 0 };
enum { WINDOW_NORMAL = 0, WINDOW_AUTOSIZE = 1 };
enum { EVENT_LBUTTONDOWN = 1 };
typedef void (*MouseCallback)(int event, int x, int y, int flags, void* userdata);

// The i-th call returns a copy of the driver's i-th image whatever the file
// name is: directory order is unspecified and must not choose the view index.
inline Mat imread(const std::string&, int = IMREAD_GRAYSCALE) {
    auto& st = standin::state();
    if (st.imread_calls >= (int)st.images.size()) throw Exception("stand-in imread: out of images");
    return st.images[st.imread_calls++].clone();
}

inline void imshow(const std::string& name, const Mat& m) { standin::state().shown[name] = m.clone(); }
inline void namedWindow(const std::string&, int = WINDOW_AUTOSIZE) {}
inline void resizeWindow(const std::string&, int, int) {}
inline void setMouseCallback(const std::string&, MouseCallback, void* = nullptr) {}
inline int waitKey(int = 0) { return -1; }

}  // namespace cv
#endif
