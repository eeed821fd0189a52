// qc_lay_frames.h — the floating frames of the layered kernels (qc_lay.hip float, qc_lay_pk.hip packed fp16).
#pragma once
#include "qc_common.h"

namespace ldpc {

// The floating frame of every block column, tabulated once per code: end[j] = the shift of the last base
// row touching column j (the frame L_j is loaded in, every sweep ends in and the outputs are stored from);
// rho[r][t] = the rotation that brings slot t's column from the frame of the row that touched it before
// (cyclically) into row r's.
template <class C>
struct LayFrames {
    struct Tab {
        int rho[C::MB][C::MAXDC], end[C::NB];
    };
    static constexpr Tab make() {
        Tab f{};
        for (int j = 0; j < C::NB; ++j) {
            int last = 0;
            for (int r = 0; r < C::MB; ++r)
                for (int t = 0; t < C::DEG[r]; ++t)
                    if (C::COL[r][t] == j) last = C::SH[r][t];
            f.end[j] = last;
            int prev = last;
            for (int r = 0; r < C::MB; ++r)
                for (int t = 0; t < C::DEG[r]; ++t)
                    if (C::COL[r][t] == j) {
                        f.rho[r][t] = (C::SH[r][t] - prev + C::Z) % C::Z;
                        prev = C::SH[r][t];
                    }
        }
        return f;
    }
    static constexpr Tab T = make();
};

}  // namespace ldpc
