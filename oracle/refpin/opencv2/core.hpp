// TEST INFRASTRUCTURE ONLY — stand-in for <opencv2/core.hpp>, written here, for compiling the reference's
// src2/matching.cpp without OpenCV (oracle/refpin/refpin_shim.cpp). matchGrid and distance use of cv::Mat
// only `rows`, `row(i)` and `ptr<int32_t>()`: a Mat here is a view of rows of bytes that the caller owns.
// The real header pulls in <cmath>, which include2/matching.h relies on (std::sqrt), so this one does too.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

namespace cv {

template <typename T> using Ptr = std::shared_ptr<T>;

class Mat {
public:
    int rows = 0, cols = 0;
    Mat() {}
    Mat(int rows_, int cols_, const unsigned char *data_, size_t step_) : rows(rows_), cols(cols_), data(data_), step(step_) {}
    Mat row(int i) const { return Mat(1, cols, data + (size_t)i * step, step); }
    template <typename T> const T *ptr(int i = 0) const { return reinterpret_cast<const T *>(data + (size_t)i * step); }

private:
    const unsigned char *data = nullptr;
    size_t step = 0;
};

}  // namespace cv
