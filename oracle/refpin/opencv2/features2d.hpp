// TEST INFRASTRUCTURE ONLY — stand-in for <opencv2/features2d.hpp>, written here: what matchNNR names, so
// that src2/matching.cpp compiles. knnMatch throws: matchNNR / match need the real BFMatcher's tie order
// and are not pinned (oracle/refpin/refpin_shim.cpp).
#pragma once

#include <stdexcept>
#include <vector>

#include "core.hpp"

namespace cv {

enum { NORM_HAMMING = 6 };

struct DMatch {
    int queryIdx = -1, trainIdx = -1, imgIdx = -1;
    float distance = 0.f;
};

class BFMatcher {
public:
    static Ptr<BFMatcher> create(int, bool) { return std::make_shared<BFMatcher>(); }
    void knnMatch(const Mat &, const Mat &, std::vector<std::vector<DMatch>> &, int) const {
        throw std::runtime_error("refpin: BFMatcher::knnMatch is a stand-in; matchNNR is not pinned");
    }
};

}  // namespace cv
