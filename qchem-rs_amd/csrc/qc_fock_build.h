// qc_fock_build.h - what the Fock build (qc_fock.hip) and the search for its stream assignment (qc_assign.hip) share.  Private to those two.
#pragma once
#include "qc_fock_kernel.h"

// timing events that are destroyed on every path out of their scope
struct EventList {
    std::vector<hipEvent_t> ev;
    int create(size_t count) {
        ev.assign(count, nullptr);
        for (auto &e : ev) if (hipEventCreate(&e) != hipSuccess) return QC_ERR_HIP;
        return QC_OK;
    }
    ~EventList() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
};

// segment of one launch: a class bucket with its slots (column kernels) or bundles (bra-major kernels)
struct Seg { const QcClass *c; const QcSlot *d_slots; int nslots; const QcBundleDev *d_bundles = nullptr; const QcKetUnit *d_ketlist = nullptr; int lds = 0; };

struct QcLaunchPlan {
    std::vector<std::vector<int>> units; std::vector<std::vector<Seg>> segs;
    std::vector<int> active() const { std::vector<int> a; for (size_t u = 0; u < units.size(); ++u) if (!units[u].empty()) a.push_back((int)u); return a; }   // units with work
};

// What the functions of one build share: the handle, the caller's arguments, the kernels' arguments made of them, the launch plan.
struct QcBuild {
    qc_system *S;
    const QcFockArgs &fa;
    const QcKernelArgs a;
    const QcLaunchPlan &plan;
    // from the first replica of the hi plane to the last replica in use of the lo plane: the planes keep the layout of QC_NREP replicas
    // whatever the number in use
    size_t accum_bytes() const { return ((fa.fxs ? fa.fx_lo : 0) + (size_t)a.nrep * a.rep_stride) * sizeof(double); }
};

// ---- qc_fock.hip (described at their definitions)
int qc_time_units_serial(const QcBuild &b, float *class_ms, float *unit_ms);
int qc_issue_build(const QcBuild &b, hipEvent_t *ev, bool per_unit, bool nofork);
// ---- qc_assign.hip
int qc_first_build(const QcBuild &b);                              // times the units alone and assigns them: the first build of a shard
bool qc_search_due(const qc_system *S, const QcFockArgs &fa);      // this build may carry an instalment of the assignment search
int qc_search_instalment(const QcBuild &b);
