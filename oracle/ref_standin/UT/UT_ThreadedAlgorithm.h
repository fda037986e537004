/* Stand-in for the HDK's UT_ThreadedAlgorithm.h: UT_ThreadedAlgorithm, UT_JobInfo and UT_Thread live with the
 * other threading helpers (one job, one processor).  See UT/UT_ParallelUtil.h. */
#ifndef REFSTANDIN_UT_THREADEDALGORITHM_H
#define REFSTANDIN_UT_THREADEDALGORITHM_H

#include <UT/UT_ParallelUtil.h>

#endif
