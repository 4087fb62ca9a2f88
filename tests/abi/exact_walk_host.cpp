// exact_walk_host.cpp -- the exact grid walk (csrc/exact_walk.hpp: cell_of, GridRows<SPARSE>::range, walk_exact) as a stand-alone
// host program, for tests/test_exact_walk_host.py (built with -ffp-contract=off -fsanitize=address,undefined).
//   exact_walk_host CASE OUT dense|sparse nearest|kth|within WANT
// CASE (little endian):
//   int32 x 8     'XWLK', points, queries, dim[0], dim[1], dim[2], 0, 0
//   float x 4     mn[0..2], 0
//   double x 2    h, inv_h
//   points  x 16  float x, y, z; uint32 original index
//   queries x 24  double x, y, z
//   queries x 8   double max2
// The program sorts the points into cells with cell_of (a stable sort: the counting sort's order inside a cell is not part of any
// contract) and builds the cell arrays of the layout itself:
//   dense   starts / counts per cell, x fastest; the grid is read from a GridMeta, as the device-decided flows read it
//   sparse  restated from seg_mark_kernel, seg_pack_kernel and seg_count_kernel (kernels_grid.hip): a segment is 16 cells along x,
//           info[s] = (occupied segments before s) << 1 | occupied, a point's cell = (info[s] >> 1) << 4 | (cx & 15), starts over
//           the cells of the occupied segments with one more entry for the end, nsegx = ceil(dim[0] / 16)
// and runs walk_exact per query with
//   nearest icp_correspond_kernel's cell (floor of the f64 value, clamped before the conversion) and candidate rule: d2 < max2,
//           the smaller d2 wins, equal d2 goes to the smaller original index
//   kth     nn_distance2_kernel's cell (cell_coord of the float) and sorted list of 2, 4 or 32 for WANT = nth + 1
//   within  cluster_link_kernel's cell (cell_coord of the float), the CONSTANT limit() = max2 and its candidate rule d2 < max2: every
//           candidate under the limit is taken, not the best one (WANT is read and ignored)
// OUT:
//   points  x 4   uint32 original index of sorted[e]
//   queries x 16  uint32 answer's index (0xFFFFFFFF: none; kth: 0), uint32 scans of this query, double answer (d2; inf: none)
//                 within: uint32 candidates taken, uint32 scans, uint32 sum (mod 2^32) and uint32 xor of their original indices --
//                 a range scanned twice, which the walk promises not to do, shows in the count
//   scans   x 16  uint32 first, uint32 last, double limit() at the scan's entry -- all queries' scans, in order
#include "exact_walk.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

using namespace cwipc_amd;

namespace {

struct Point { float x, y, z; uint32_t id; };
struct Answer { uint32_t id, scans; double d2; };
struct ScanRec { uint32_t first, last; double limit; };

struct Case {
    Grid g;
    std::vector<Point> pts;
    std::vector<double> q, max2;
};

bool read_case(const char *path, Case &c) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    int32_t hdr[8];
    float mn[4];
    double hh[2];
    bool ok = fread(hdr, sizeof(hdr), 1, f) == 1 && fread(mn, sizeof(mn), 1, f) == 1 && fread(hh, sizeof(hh), 1, f) == 1;
    ok = ok && hdr[0] == 0x4B4C5758 && hdr[1] >= 0 && hdr[2] >= 0 && hdr[3] >= 1 && hdr[4] >= 1 && hdr[5] >= 1;
    if (ok) {
        for (int a = 0; a < 3; a++) { c.g.mn[a] = mn[a]; c.g.dim[a] = hdr[3 + a]; }
        c.g.h = hh[0];
        c.g.inv_h = hh[1];
        c.g.nsegx = (c.g.dim[0] + SEG - 1) / SEG;
        c.pts.resize((size_t)hdr[1]);
        c.q.resize((size_t)hdr[2] * 3);
        c.max2.resize((size_t)hdr[2]);
        ok = (c.pts.empty() || fread(c.pts.data(), sizeof(Point), c.pts.size(), f) == c.pts.size()) &&
             (c.q.empty() || fread(c.q.data(), sizeof(double), c.q.size(), f) == c.q.size()) &&
             (c.max2.empty() || fread(c.max2.data(), sizeof(double), c.max2.size(), f) == c.max2.size());
    }
    fclose(f);
    return ok;
}

// The points in cell order and the layout's two arrays.
struct Cells {
    std::vector<Point> sorted;
    std::vector<uint32_t> starts, counts;
};

void sort_by(const std::vector<Point> &pts, const std::vector<uint32_t> &cell, size_t ncell, Cells &out) {
    std::vector<uint32_t> order(pts.size());
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cell[a] < cell[b]; });
    out.sorted.resize(pts.size());
    for (size_t e = 0; e < pts.size(); e++) out.sorted[e] = pts[order[e]];
    std::vector<uint32_t> per(ncell, 0u);
    for (uint32_t c : cell) per[c]++;
    out.starts.assign(ncell + 1, 0u);
    for (size_t c = 0; c < ncell; c++) out.starts[c + 1] = out.starts[c] + per[c];
    out.counts = per;
}

void build_dense(const Case &c, Cells &out) {
    const Grid &g = c.g;
    std::vector<uint32_t> cell(c.pts.size());
    for (size_t i = 0; i < c.pts.size(); i++) cell[i] = cell_of(g, c.pts[i].x, c.pts[i].y, c.pts[i].z);
    sort_by(c.pts, cell, (size_t)g.dim[0] * (size_t)g.dim[1] * (size_t)g.dim[2], out);
    out.starts.pop_back();   // starts / counts per cell
}

void build_sparse(const Case &c, Cells &out) {
    const Grid &g = c.g;
    const size_t nseg = (size_t)g.nsegx * (size_t)g.dim[1] * (size_t)g.dim[2];
    std::vector<uint32_t> segcell(c.pts.size()), masks(nseg, 0u);
    for (size_t i = 0; i < c.pts.size(); i++) {   // seg_cell_of, seg_mark_kernel
        const uint32_t cx = (uint32_t)cell_coord(g, c.pts[i].x, 0);
        const uint32_t seg = (cx >> SEG_SHIFT) + (uint32_t)g.nsegx * ((uint32_t)cell_coord(g, c.pts[i].y, 1) + (uint32_t)g.dim[1] * (uint32_t)cell_coord(g, c.pts[i].z, 2));
        segcell[i] = (seg << SEG_SHIFT) | (cx & (SEG - 1));
        masks[seg] |= 1u << (cx & (SEG - 1));
    }
    std::vector<uint32_t> info(nseg);
    uint32_t before = 0;
    for (size_t s = 0; s < nseg; s++) {   // seg_pack_kernel
        const uint32_t flag = masks[s] != 0u;
        info[s] = (before << 1) | flag;
        before += flag;
    }
    std::vector<uint32_t> cell(c.pts.size());
    for (size_t i = 0; i < c.pts.size(); i++) cell[i] = ((info[segcell[i] >> SEG_SHIFT] >> 1) << SEG_SHIFT) | (segcell[i] & (SEG - 1));   // seg_count_kernel
    sort_by(c.pts, cell, (size_t)before << SEG_SHIFT, out);
    out.counts = info;   // the segment table is what a sparse GridView calls counts
}

struct Out {
    std::vector<Answer> answers;
    std::vector<ScanRec> scans;
};

template <bool SPARSE>
void run_nearest(const Case &cs, const GridRows<SPARSE> &rows, const Cells &cells, Out &out) {
    const Grid &g = rows.g;
    const Point *sorted = cells.sorted.data();
    for (size_t qi = 0; qi < cs.max2.size(); qi++) {
        const double q[3] = {cs.q[3 * qi], cs.q[3 * qi + 1], cs.q[3 * qi + 2]};
        const double max2 = cs.max2[qi];
        int c[3];
        for (int a = 0; a < 3; a++) {
            double f = floor((q[a] - (double)g.mn[a]) * g.inv_h);
            f = f < 0.0 ? 0.0 : f;
            c[a] = f >= (double)g.dim[a] ? g.dim[a] - 1 : (int)f;
        }
        double best = INFINITY;
        uint32_t best_idx = 0xFFFFFFFFu, nscan = 0;
        auto limit = [&]() { return fmin(best, max2); };
        auto scan = [&](uint32_t first, uint32_t last) {
            out.scans.push_back(ScanRec{first, last, limit()});
            nscan++;
            for (uint32_t e = first; e < last; e++) {
                const Point &p = sorted[e];
                const double dx = q[0] - (double)p.x, dy = q[1] - (double)p.y, dz = q[2] - (double)p.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < max2 && (d2 < best || (d2 == best && p.id < best_idx))) {
                    best = d2;
                    best_idx = p.id;
                }
            }
        };
        walk_exact(rows, q, c, limit, scan);
        out.answers.push_back(Answer{best_idx, nscan, best_idx == 0xFFFFFFFFu ? (double)INFINITY : best});
    }
}

template <int KCAP, bool SPARSE>
void run_kth(const Case &cs, const GridRows<SPARSE> &rows, const Cells &cells, int want, Out &out) {
    const Grid &g = rows.g;
    const Point *sorted = cells.sorted.data();
    for (size_t qi = 0; qi < cs.max2.size(); qi++) {
        const float qf[3] = {(float)cs.q[3 * qi], (float)cs.q[3 * qi + 1], (float)cs.q[3 * qi + 2]};
        const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
        const double max2 = cs.max2[qi];
        const int c[3] = {cell_coord(g, qf[0], 0), cell_coord(g, qf[1], 1), cell_coord(g, qf[2], 2)};
        const int pad = KCAP - want;
        double best[KCAP];
        for (int j = 0; j < KCAP; j++) best[j] = j < pad ? -INFINITY : INFINITY;
        uint32_t nscan = 0;
        auto limit = [&]() { return fmin(best[KCAP - 1], max2); };
        auto scan = [&](uint32_t first, uint32_t last) {
            out.scans.push_back(ScanRec{first, last, limit()});
            nscan++;
            for (uint32_t e = first; e < last; e++) {
                const Point &p = sorted[e];
                const double dx = q[0] - (double)p.x, dy = q[1] - (double)p.y, dz = q[2] - (double)p.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < limit()) {
                    for (int j = KCAP - 1; j >= 1; j--) best[j] = d2 < best[j - 1] ? best[j - 1] : fmin(best[j], d2);
                    best[0] = fmin(best[0], d2);
                }
            }
        };
        walk_exact(rows, q, c, limit, scan);
        out.answers.push_back(Answer{0u, nscan, best[KCAP - 1]});
    }
}

template <bool SPARSE>
void run_within(const Case &cs, const GridRows<SPARSE> &rows, const Cells &cells, Out &out) {
    const Grid &g = rows.g;
    const Point *sorted = cells.sorted.data();
    for (size_t qi = 0; qi < cs.max2.size(); qi++) {
        const float qf[3] = {(float)cs.q[3 * qi], (float)cs.q[3 * qi + 1], (float)cs.q[3 * qi + 2]};
        const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
        const double max2 = cs.max2[qi];
        const int c[3] = {cell_coord(g, qf[0], 0), cell_coord(g, qf[1], 1), cell_coord(g, qf[2], 2)};
        uint32_t taken = 0, sum = 0, x = 0, nscan = 0;
        auto limit = [&]() { return max2; };
        auto scan = [&](uint32_t first, uint32_t last) {
            out.scans.push_back(ScanRec{first, last, limit()});
            nscan++;
            for (uint32_t e = first; e < last; e++) {
                const Point &p = sorted[e];
                const double dx = q[0] - (double)p.x, dy = q[1] - (double)p.y, dz = q[2] - (double)p.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 < max2)) continue;
                taken++;
                sum += p.id;
                x ^= p.id;
            }
        };
        walk_exact(rows, q, c, limit, scan);
        Answer a{taken, nscan, 0.0};
        const uint32_t words[2] = {sum, x};
        memcpy(&a.d2, words, sizeof(words));
        out.answers.push_back(a);
    }
}

template <bool SPARSE>
void run(const Case &cs, const GridRows<SPARSE> &rows, const Cells &cells, const char *kind, int want, Out &out) {
    const bool nearest = !strcmp(kind, "nearest");
    if (!strcmp(kind, "within")) run_within(cs, rows, cells, out);
    else if (nearest) run_nearest(cs, rows, cells, out);
    else if (want <= 2) run_kth<2>(cs, rows, cells, want, out);
    else if (want <= 4) run_kth<4>(cs, rows, cells, want, out);
    else run_kth<32>(cs, rows, cells, want, out);
}

}  // namespace

int main(int argc, char **argv) {
    const bool usage = argc == 6 && (!strcmp(argv[3], "dense") || !strcmp(argv[3], "sparse")) && (!strcmp(argv[4], "nearest") || !strcmp(argv[4], "kth") || !strcmp(argv[4], "within"));
    const int want = usage ? atoi(argv[5]) : 0;
    if (!usage || want < 1 || want > 32) {
        fprintf(stderr, "usage: exact_walk_host CASE OUT dense|sparse nearest|kth|within WANT(1..32)\n");
        return 2;
    }
    Case cs;
    if (!read_case(argv[1], cs)) {
        fprintf(stderr, "exact_walk_host: cannot read the case %s\n", argv[1]);
        return 2;
    }
    const bool sparse = !strcmp(argv[3], "sparse");
    Cells cells;
    Out out;
    if (sparse) {
        build_sparse(cs, cells);
        const GridRows<true> rows(cs.g, nullptr, cells.starts.data(), cells.counts.data(), nullptr);
        run(cs, rows, cells, argv[4], want, out);
    } else {
        build_dense(cs, cells);
        GridMeta meta{};
        meta.g = cs.g;
        const GridRows<false> rows(Grid{}, &meta, cells.starts.data(), cells.counts.data(), nullptr);
        run(cs, rows, cells, argv[4], want, out);
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) return 3;
    std::vector<uint32_t> ids(cells.sorted.size());
    for (size_t e = 0; e < ids.size(); e++) ids[e] = cells.sorted[e].id;
    bool ok = (ids.empty() || fwrite(ids.data(), sizeof(uint32_t), ids.size(), f) == ids.size()) &&
              (out.answers.empty() || fwrite(out.answers.data(), sizeof(Answer), out.answers.size(), f) == out.answers.size()) &&
              (out.scans.empty() || fwrite(out.scans.data(), sizeof(ScanRec), out.scans.size(), f) == out.scans.size());
    ok = fclose(f) == 0 && ok;
    return ok ? 0 : 3;
}
