// pe_pathfinder.hpp -- the scripted path-finding pursuers of Pursuit_Env (include/pe_env.h pe_pursuer_pathfinder; DESIGN.md section
// 7n; plain-Python restatement and authority: tests/pe_pathfinder_ref.py), shared by the kernel and the host twin.  Included by
// pe_env.hip after the tick's own helpers: py_round, in_bound_i, div_const, dynamic, probe_hit and walk_clear are the tick's, used
// here as they stand, so a candidate's look-ahead is the very arithmetic dev_step applies to the chosen action.
//
// Per environment: s = cell(evader), D = least fixed point of
//   D[s] = 0,  D[c] = min over admissible neighbours n of step(c, n) + pen(n) + D[n]   (free c != s; PE_PATH_UNREACHED elsewhere)
// with step 10 / 14, no corner cutting and pen(n) = clearance on cells n != s that touch an occupied cell.  Per cell the kernel keeps
// one 16-bit neighbour word (bit k: neighbour k is admissible, bit 8 + k: it carries the penalty), so relaxing a cell reads the word
// and at most eight distances.  All integers: any relaxation order gives the same field.
// Plain *, +, -, /, sqrt in the order written; the translation unit is built with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

namespace {
namespace pepath {

constexpr int32_t UNREACHED = PE_PATH_UNREACHED;
constexpr int THREADS = 256;   // one workgroup of four waves per environment

// neighbour k lies in direction k pi / 4: (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1)
__host__ __device__ __forceinline__ int dir_dx(int k) { return (k == 0 || k == 1 || k == 7) ? 1 : ((k >= 3 && k <= 5) ? -1 : 0); }
__host__ __device__ __forceinline__ int dir_dy(int k) { return (k >= 1 && k <= 3) ? 1 : (k >= 5 ? -1 : 0); }

__host__ __device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__host__ __device__ __forceinline__ double clampd(double v, double hi) { return v < 0.0 ? 0.0 : (v > hi ? hi : v); }
// cell(x, y) = (clamp(py_round(x), 0, W - 1), clamp(py_round(y), 0, H - 1)) as the grid index x H + y
__host__ __device__ __forceinline__ int cell_id(const pe_config &c, double x, double y) {
    return clampi(py_round(x), c.W - 1) * c.H + clampi(py_round(y), c.H - 1);
}

// pen(n) != 0: n is not the source and one of its eight in-map neighbours is occupied
__host__ __device__ inline uint8_t pen_cell(const pe_config &c, const uint8_t *grid, int x, int y, int s) {
    if (x * c.H + y == s) return 0;
    for (int k = 0; k < 8; k++) {
        const int nx = x + dir_dx(k), ny = y + dir_dy(k);
        if (in_bound_i(c, nx, ny) && grid[nx * c.H + ny] != 0) return 1;
    }
    return 0;
}

// admissibility: the neighbour word of cell (x, y).  Neighbour k is admissible when it is in the map and free or the source; a
// diagonal one also needs both cells that share the corner free.  Occupied cells other than the source have no neighbours.
__host__ __device__ inline uint16_t neighbour_word(const pe_config &c, const uint8_t *grid, const uint8_t *pen, int x, int y, int s) {
    const int H = c.H, id = x * H + y;
    if (grid[id] != 0 && id != s) return 0;
    uint32_t w = 0;
    for (int k = 0; k < 8; k++) {
        const int dx = dir_dx(k), dy = dir_dy(k), nx = x + dx, ny = y + dy;
        if (!in_bound_i(c, nx, ny)) continue;
        const int n = nx * H + ny;
        if (grid[n] != 0 && n != s) continue;
        if ((k & 1) && (grid[nx * H + y] != 0 || grid[x * H + ny] != 0)) continue;
        w |= 1u << k;
        if (pen[n]) w |= 1u << (8 + k);
    }
    return (uint16_t)w;
}

// relax one cell: min over its admissible, reached neighbours of step + pen + D, and the first direction that attains it (8 = none)
__host__ __device__ __forceinline__ int32_t relax_cell(uint32_t w, const int32_t *D, int id, int H, int32_t clearance, int *kbest) {
    int32_t best = UNREACHED;
    int kb = 8;
    for (int k = 0; k < 8; k++) {
        if (!((w >> k) & 1u)) continue;
        const int32_t dn = D[id + dir_dx(k) * H + dir_dy(k)];
        if (dn == UNREACHED) continue;
        const int32_t v = dn + ((k & 1) ? 14 : 10) + (((w >> (8 + k)) & 1u) ? clearance : 0);
        if (v < best) { best = v; kb = k; }
    }
    *kbest = kb;
    return best;
}

// the desired heading k* of a pursuer at (px, py): 0..7, or 8 for none.  e = the evader's record (x, y, vx, vy).
__host__ __device__ inline int heading(const pe_config &c, const uint8_t *grid, const int32_t *D, const uint16_t *nb,
                                       const pe_pathfinder_params &prm, double px, double py, const double *e) {
    const int H = c.H;
    const double wmax = (double)(c.W - 1), hmax = (double)(c.H - 1);
    const int ci = cell_id(c, px, py);
    const double dx = e[0] - px, dy = e[1] - py;
    const double d = __builtin_sqrt(dx * dx + dy * dy);
    double t = d / c.action_u[0][0];
    if (t > prm.lead) t = prm.lead;
    double ax = clampd(e[0] + t * e[2], wmax), ay = clampd(e[1] + t * e[3], hmax);
    int ai = cell_id(c, ax, ay);
    if (grid[ai] != 0) { ax = e[0]; ay = e[1]; ai = cell_id(c, ax, ay); }
    bool direct = true;
    if (D[ci] == UNREACHED) { ax = e[0]; ay = e[1]; }
    else direct = walk_clear<false>(grid, H, ci / H, ci % H, ai / H, ai % H, 4 * (c.W + c.H));
    if (direct) {
        const double vx = ax - px, vy = ay - py;
        if (vx * vx + vy * vy <= 1e-4) return 8;
        int best = 0;
        double bd = vx * c.action_u[0][0] + vy * c.action_u[0][1];
        for (int k = 1; k < 8; k++) {
            const double dk = vx * c.action_u[k][0] + vy * c.action_u[k][1];
            if (dk > bd) { bd = dk; best = k; }
        }
        return best;
    }
    int kb;
    relax_cell(nb[ci], D, ci, H, prm.clearance, &kb);
    return kb;
}

// the candidate order: k*, k* + 1, k* - 1, k* + 2, k* - 2, k* + 3, k* - 3, k* + 4 (mod 8), then 8; with k* = 8: 8, then 0..7
__host__ __device__ __forceinline__ int candidate(int kstar, int idx) {
    if (kstar == 8) return idx == 0 ? 8 : idx - 1;
    if (idx == 8) return 8;
    const int off = (idx & 1) ? (idx + 1) >> 1 : -(idx >> 1);
    return (kstar + off) & 7;
}

// one (pursuer, candidate) pair: the tick's lag integration of action k, the tick's 3 x 3 probe on the proposal, and the
// right-of-way test against the lower-indexed team-mates.  def = the environment's record x[P], y[P], vx[P], vy[P].
__host__ __device__ inline void candidate_flags(const pe_config &c, double itau, double i6, const uint8_t *grid, const double *def, int i, int k,
                                                double sep2, bool *blocked, bool *crowded) {
    const int P = c.P;
    const double x = def[i], y = def[P + i];
    double q[4];
    dynamic(c.def_tau, itau, i6, c.def_dt, x, y, def[2 * P + i], def[3 * P + i], c.action_u[k][0], c.action_u[k][1], q);
    bool hit = false;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) hit = hit || probe_hit(c, grid, q[0], q[1], a - 1, b - 1, c.def_collision_radius);
    bool near = false;
    for (int j = 0; j < i; j++) {
        const double qx = q[0] - def[j], qy = q[1] - def[P + j], ox = x - def[j], oy = y - def[P + j];
        const double nq = qx * qx + qy * qy, no = ox * ox + oy * oy;
        near = near || (nq <= sep2 && nq < no);
    }
    *blocked = hit;
    *crowded = near;
}

// the choice: the first candidate neither blocked nor crowded, failing that the first not blocked, failing that 8
__host__ __device__ inline int choose(int kstar, uint32_t blocked, uint32_t crowded) {
    for (int idx = 0; idx < 9; idx++) {
        const int k = candidate(kstar, idx);
        if (!(((blocked | crowded) >> k) & 1u)) return k;
    }
    for (int idx = 0; idx < 9; idx++) {
        const int k = candidate(kstar, idx);
        if (!((blocked >> k) & 1u)) return k;
    }
    return 8;
}

// the penalty bits and neighbour words of source s: all a cached field needs rebuilt around it (they depend on s, two passes)
inline void words_host(const pe_config &c, const uint8_t *grid, int s, uint8_t *pen, uint16_t *nb) {
    const int W = c.W, H = c.H;
    for (int x = 0; x < W; x++)
        for (int y = 0; y < H; y++) pen[x * H + y] = pen_cell(c, grid, x, y, s);
    for (int x = 0; x < W; x++)
        for (int y = 0; y < H; y++) nb[x * H + y] = neighbour_word(c, grid, pen, x, y, s);
}

// the host's schedule: in-place sweeps, forwards and backwards in turn, until one changes nothing.  Returns the sweeps, -1 at the bound.
inline int field_host(const pe_config &c, const uint8_t *grid, int s, int32_t clearance, int32_t *D, uint8_t *pen, uint16_t *nb) {
    const int H = c.H, WH = c.W * H;
    words_host(c, grid, s, pen, nb);
    for (int id = 0; id < WH; id++) D[id] = UNREACHED;
    D[s] = 0;
    for (int sweep = 0; sweep < WH; sweep++) {
        bool changed = false;
        for (int q = 0; q < WH; q++) {
            const int id = (sweep & 1) ? WH - 1 - q : q;
            if (id == s || nb[id] == 0) continue;
            int kb;
            const int32_t v = relax_cell(nb[id], D, id, H, clearance, &kb);
            if (v < D[id]) { D[id] = v; changed = true; }
        }
        if (!changed) return sweep + 1;
    }
    return -1;
}

__host__ __device__ inline size_t lds_bytes(int WH, int P) {
    return sizeof(double) * (4 * P + 4) + sizeof(int32_t) * (size_t)WH + sizeof(uint16_t) * (size_t)WH + 2 * (((size_t)WH + 15) & ~(size_t)15) +
           16 * sizeof(int32_t) + sizeof(int32_t) * PE_MAX_P + 2 * 16 * PE_MAX_P;
}

}  // namespace pepath
}  // namespace
