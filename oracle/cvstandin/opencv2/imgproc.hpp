// Stand-in for <opencv2/imgproc.hpp>: resize only (see core.hpp in this folder).
#ifndef SVA_CVSTANDIN_IMGPROC_HPP
#define SVA_CVSTANDIN_IMGPROC_HPP

#include "core.hpp"

namespace cv {

// Bilinear resize with pixel centres aligned, edges clamped, f64 arithmetic;
// u8 results round to nearest.  dsize wins when it is non-empty, otherwise the
// size is (cvRound(cols * fx), cvRound(rows * fy)).  src and dst may be the
// same Mat.  The fixtures never depend on this rule: the driver only feeds it
// images whose 2x2 blocks are constant.
inline void resize(const Mat& src, Mat& dst, Size dsize, double fx = 0, double fy = 0) {
    if (src.empty()) throw Exception("stand-in resize: empty source");
    if (dsize.width <= 0 || dsize.height <= 0)
        dsize = Size(cvRound(src.cols * fx), cvRound(src.rows * fy));
    if (dsize.width <= 0 || dsize.height <= 0) throw Exception("stand-in resize: empty size");
    const double sx = (double)src.cols / dsize.width, sy = (double)src.rows / dsize.height;
    Mat out(dsize.height, dsize.width, src.type());
    for (int y = 0; y < dsize.height; y++) {
        double fy_ = (y + 0.5) * sy - 0.5;
        int y0 = (int)std::floor(fy_);
        double wy = fy_ - y0;
        int ya = std::min(std::max(y0, 0), src.rows - 1), yb = std::min(std::max(y0 + 1, 0), src.rows - 1);
        for (int x = 0; x < dsize.width; x++) {
            double fx_ = (x + 0.5) * sx - 0.5;
            int x0 = (int)std::floor(fx_);
            double wx = fx_ - x0;
            int xa = std::min(std::max(x0, 0), src.cols - 1), xb = std::min(std::max(x0 + 1, 0), src.cols - 1);
            double top = src.get(ya, xa) * (1.0 - wx) + src.get(ya, xb) * wx;
            double bot = src.get(yb, xa) * (1.0 - wx) + src.get(yb, xb) * wx;
            double v = top * (1.0 - wy) + bot * wy;
            switch (src.type()) {
                case CV_8U: out.at<uint8_t>(y, x) = (uint8_t)std::min(255, std::max(0, cvRound(v))); break;
                case CV_32F: out.at<float>(y, x) = (float)v; break;
                default: out.at<double>(y, x) = v;
            }
        }
    }
    dst = out;
}

}  // namespace cv
#endif
