// run_level2_gpu.cpp with a waterfall detector: the same scripted server loop (hip_level2.h on the real HipFanout and
// libpsdr_hip.so), but every HipFanout is created with Params::waterfall_detector = PSDR_TEST_WF_DETECTOR - what a
// server does with input.waterfall_detector.  tests/test_gpu_level2_wf_detector.py compares what
// reaches the mock waterfall encoders with the detector's contract.
//
//   g++ -DPSDR_TEST_WF_DETECTOR=PSDR_WF_PEAK ... run_level2_wf_detector.cpp
#include "hip_fanout.h"

#ifndef PSDR_TEST_WF_DETECTOR
#error "define PSDR_TEST_WF_DETECTOR (PSDR_WF_PEAK or PSDR_WF_MEAN)"
#endif

class DetectorFanout : public HipFanout {
  public:
    explicit DetectorFanout(const Params &p) : HipFanout(with_detector(p)) {}

  private:
    static Params with_detector(Params p) {
        p.waterfall_detector = PSDR_TEST_WF_DETECTOR;
        return p;
    }
};

#define HipFanout DetectorFanout
#include "run_level2_gpu.cpp"
