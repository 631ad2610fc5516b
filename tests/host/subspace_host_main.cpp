// subspace_host_main.cpp - a stand-alone driver of the host numerics of the reduced-space solvers (qc_subspace_host.h) for
// tests/test_subspace_host.py: built with the system C++ compiler and its address and undefined-behaviour sanitizers, no HIP.
//   subspace_host_main <eig|lu|tdhf|gs> <in> <out>      both files: raw float64
//   eig   in [m, rel_stop, A (m x m)]                   out [w (m), Vr (m x m, rows = eigenvectors)]
//   lu    in [m, nrhs, A (m x m), b (nrhs x m)]         out [ok, y (nrhs x m)]
//   tdhf  in [m, nroots, Mp (m x m), Mm (m x m)]        out [ok, omega (nroots), Rt (nroots x m), Lt (nroots x m)]
//   gs    in [ld, m, nsrc, src (nsrc x m)]              out [rows kept, per source: kept (1), row k of Z as the call left it (ld)]
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "qc_subspace_host.h"

static std::vector<double> read_all(const char *path) {
    std::vector<double> x;
    FILE *f = std::fopen(path, "rb");
    if (!f) return x;
    double buf[512];
    size_t n;
    while ((n = std::fread(buf, sizeof(double), 512, f)) > 0) x.insert(x.end(), buf, buf + n);
    std::fclose(f);
    return x;
}

int main(int argc, char **argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s <eig|lu|tdhf|gs> <in> <out>\n", argv[0]); return 2; }
    const std::string op = argv[1];
    const std::vector<double> in = read_all(argv[2]);
    std::vector<double> out;
    if (op == "eig" && in.size() >= 2) {
        const int m = (int)in[0];
        if (in.size() != 2 + (size_t)m * m) return 3;
        std::vector<double> A(in.begin() + 2, in.end()), w, Vr;
        host_sym_eig(m, A, w, Vr, in[1]);
        out = w; out.insert(out.end(), Vr.begin(), Vr.end());
    } else if (op == "lu" && in.size() >= 2) {
        const int m = (int)in[0], nrhs = (int)in[1];
        if (in.size() != 2 + (size_t)m * m + (size_t)nrhs * m) return 3;
        std::vector<double> A(in.begin() + 2, in.begin() + 2 + (size_t)m * m), y((size_t)nrhs * m, 0.0);
        const bool ok = host_lu_solve(m, A, nrhs, in.data() + 2 + (size_t)m * m, y.data());
        out.push_back(ok ? 1.0 : 0.0); out.insert(out.end(), y.begin(), y.end());
    } else if (op == "tdhf" && in.size() >= 2) {
        const int m = (int)in[0], nroots = (int)in[1];
        if (in.size() != 2 + 2 * (size_t)m * m) return 3;
        std::vector<double> Mp(in.begin() + 2, in.begin() + 2 + (size_t)m * m), Mm(in.begin() + 2 + (size_t)m * m, in.end()), Rt, Lt, omega(nroots, 0.0);
        const bool ok = tdhf_reduced(m, Mp, Mm, nroots, omega.data(), Rt, Lt);
        Rt.resize((size_t)nroots * m, 0.0); Lt.resize((size_t)nroots * m, 0.0);
        out.push_back(ok ? 1.0 : 0.0);
        out.insert(out.end(), omega.begin(), omega.end()); out.insert(out.end(), Rt.begin(), Rt.end()); out.insert(out.end(), Lt.begin(), Lt.end());
    } else if (op == "gs" && in.size() >= 3) {
        const int ld = (int)in[0], m = (int)in[1], nsrc = (int)in[2];
        if (in.size() != 3 + (size_t)nsrc * m || m > ld) return 3;
        std::vector<double> Z((size_t)(nsrc + 1) * ld, 0.0);
        int k = 0;
        out.push_back(0.0);
        for (int s = 0; s < nsrc; ++s) {
            const bool kept = qc_orthonormalize_row(Z.data(), ld, m, k, in.data() + 3 + (size_t)s * m);
            out.push_back(kept ? 1.0 : 0.0);
            out.insert(out.end(), Z.begin() + (size_t)k * ld, Z.begin() + (size_t)(k + 1) * ld);
            if (kept) ++k;
        }
        out[0] = k;
    } else {
        return 2;
    }
    FILE *f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 4;
    std::fclose(f);
    return 0;
}
