// qc_rccl.cpp - the RCCL run-time loader (QcRccl, qc_internal.h).
#include <dlfcn.h>

#include <cstdlib>

#include "qc_internal.h"

// ---- RCCL, bound at run time.  A process that has imported torch already maps torch's bundled librccl.so.1; linking a
// second copy by path would leave it to the dynamic loader which of the two same-soname libraries the symbols resolve to.
// The library is therefore not linked: the first qc_comm_* call takes (1) $QC_RCCL_LIB if set, else (2) the librccl.so.1
// already mapped into the process (one RCCL per process: torch's, when torch is there), else (3) librccl.so.1 from the
// loader's search path (rpath /opt/rocm/lib).  qc_rccl_info() reports which one it was.
QcRccl &qc_rccl() {
    // (on the heap and never destroyed: a handle with a communicator may be released after the static destructors have run)
    static QcRccl &R = *new QcRccl([] {
        QcRccl r;
        const char *env = getenv("QC_RCCL_LIB");
        if (env && *env) { r.handle = dlopen(env, RTLD_NOW | RTLD_GLOBAL); r.path = env; }
        if (!r.handle) { r.handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD); r.path = "librccl.so.1 (already mapped in this process)"; }
        if (!r.handle) { r.handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL); r.path = "librccl.so.1 (loader search path)"; }
        if (!r.handle) { fprintf(stderr, "qchem_hip: cannot load librccl.so.1: %s\n", dlerror()); return r; }
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.handle, "ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.handle, "ncclCommInitRank"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.handle, "ncclCommDestroy"));
        r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(r.handle, "ncclAllReduce"));
        r.GetVersion = reinterpret_cast<decltype(r.GetVersion)>(dlsym(r.handle, "ncclGetVersion"));
        r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllReduce;
        if (r.ok) {
            Dl_info info;
            if (dladdr(reinterpret_cast<void *>(r.AllReduce), &info) && info.dli_fname) r.path = info.dli_fname;
        }
        return r;
    }());
    return R;
}
