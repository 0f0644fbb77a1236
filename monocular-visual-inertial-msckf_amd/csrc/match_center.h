// The centre of a track's search window in the newest frame, PREDICTED from what the engine holds at match time (NOT in the
// reference).  Today the window of msckf_tracks_set_match_options is centred on the track's last stored keypoint.
//
// THE RULE.  R_n, t_n: the resident pose of the newest clone (slot N - 1) when the match runs; K: the caller's intrinsics,
// row-major.  project(w): c = R_n^T w, h = K c, the centre (h_x / h_z, h_y / h_z); defined iff h_z > 0 and both are finite.
//   ROTATED  w = d, the stored direction of the track's last view (R_l K^-1 [u v 1], not normalised): the last keypoint carried
//            through the rotation between its clone and the newest one, the translation ignored
//   POINT    w = rho (base - t_n) + m, the track's inverse-depth point seen from the newest clone (view_row.h's w); defined
//            only for a triangulated track with rho > 0
// Mode POINT takes ROTATED where POINT is undefined; a track whose ROTATED centre is undefined has NO centre: both components
// are NaN, which no keypoint is within any radius of.  how: 0 the last keypoint (mode LAST), 1 rotated, 2 point, 3 none.
//
// Host and device code from one text, without a HIP header and on plain pointers and scalars, in the manner of view_row.h:
// tests/test_match_center.py compiles it with the host compiler (and its sanitizers) against the NumPy restatement in
// tests/match_center_ref.py.  No kernel calls it yet: the rule, its tolerance and its scenes stand first.
#pragma once

#if defined(__HIPCC__)
#define MSCKF_CENTER_HD __host__ __device__ __forceinline__
#else
#define MSCKF_CENTER_HD inline
#endif

namespace msckf {

constexpr int MATCH_CENTER_LAST = 0, MATCH_CENTER_ROTATED = 1, MATCH_CENTER_POINT = 2;          // the modes
constexpr int MATCH_HOW_LAST = 0, MATCH_HOW_ROTATED = 1, MATCH_HOW_POINT = 2, MATCH_HOW_NONE = 3;

// project(w) into uv[2]; false (uv untouched): undefined
MSCKF_CENTER_HD bool match_center_project(const double* Rn, const double* K, double wx, double wy, double wz, double* uv) {
    const double cx = Rn[0] * wx + Rn[3] * wy + Rn[6] * wz;
    const double cy = Rn[1] * wx + Rn[4] * wy + Rn[7] * wz;
    const double cz = Rn[2] * wx + Rn[5] * wy + Rn[8] * wz;
    const double hx = K[0] * cx + K[1] * cy + K[2] * cz;
    const double hy = K[3] * cx + K[4] * cy + K[5] * cz;
    const double hz = K[6] * cx + K[7] * cy + K[8] * cz;
    if (!(hz > 0.0)) return false;
    const double u = hx / hz, v = hy / hz;
    if (!__builtin_isfinite(u) || !__builtin_isfinite(v)) return false;
    uv[0] = u; uv[1] = v;
    return true;
}

// mode: ROTATED or POINT.  d [3]: the last view's direction; base, m [3], rho: the track's point, base resolved as a batch
// resolves it (the anchor clone's resident position, or the frozen one); triangulated: a selection run refreshed that point.
// Returns how and writes uv[2] (NaN, NaN for how = 3).
MSCKF_CENTER_HD int match_center(int mode, const double* Rn, const double* tn, const double* K, const double* d, const double* base,
                                 const double* m, double rho, bool triangulated, double* uv) {
    if (mode == MATCH_CENTER_POINT && triangulated && rho > 0.0) {
        const double wx = rho * (base[0] - tn[0]) + m[0];
        const double wy = rho * (base[1] - tn[1]) + m[1];
        const double wz = rho * (base[2] - tn[2]) + m[2];
        if (match_center_project(Rn, K, wx, wy, wz, uv)) return MATCH_HOW_POINT;
    }
    if (match_center_project(Rn, K, d[0], d[1], d[2], uv)) return MATCH_HOW_ROTATED;
    uv[0] = uv[1] = __builtin_nan("");
    return MATCH_HOW_NONE;
}

}  // namespace msckf
