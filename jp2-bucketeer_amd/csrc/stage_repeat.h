// stage_repeat.h -- stage-cost experiments (tests/tools/stage_cost2.sh) build
// with -DJP2HIP_REPEAT_STAGE=<n> to launch one stage's kernels twice (they are
// idempotent): 1 DWT, 2 quantiser, 3 MQ, 4 hull, 5 tier-2 sizing wave kernel.
// Product builds never define it.
#pragma once

#ifndef JP2HIP_REPEAT_STAGE
#define JP2HIP_REPEAT_STAGE 0
#endif
#define REPEAT_IF(n) for (int rep_ = 0; rep_ < (JP2HIP_REPEAT_STAGE == (n) ? 2 : 1); rep_++)
