// voxel_anchor_host.cpp -- the downsample's host arithmetic (csrc/voxel_anchor.hpp: anchor box, face thresholds, range plans)
// compiled for the host, for tests/test_voxel_anchor_host.py.  The set-up of a call is restated from voxel_downsample()'s plan
// and anchor steps: inv_leaf = 1 / cellsize in fp32, octree resolution (double)(float)(64 * cellsize), faces from 1 - FACE_BACK.
#include "voxel_anchor.hpp"

using namespace cwipc_amd;

extern "C" {

// K1_WAVES, WAVE_STEP, MAX_POINTS_PER_WAVE, FACES, FT_T, FT_TV, FT_TF, FACE_TABLE_WORDS
void voxel_constants(long out[8]) {
    const long v[8] = {K1_WAVES, WAVE_STEP, (long)MAX_POINTS_PER_WAVE, FACES, FT_T, FT_TV, FT_TF, FACE_TABLE_WORDS};
    for (int i = 0; i < 8; i++) out[i] = v[i];
}

// The face table of a cloud whose first point is `anchor`: table[FACE_TABLE_WORDS], the anchor box's lower corner, the resolution,
// inv_leaf and the number of the table's first face per axis.
void voxel_face_table(const float anchor[3], float cellsize, uint32_t *table, double mn0[3], double *res, float *inv_leaf, int face_base[3]) {
    *inv_leaf = 1.0f / cellsize;
    const float octree_cellsize = (8 * 8) * cellsize;
    *res = (double)octree_cellsize;
    const double pp[3] = {(double)anchor[0], (double)anchor[1], (double)anchor[2]};
    double mx0[3];
    int depth0;
    first_box(pp, *res, mn0, mx0, depth0);
    for (int a = 0; a < 3; a++) face_base[a] = 1 - FACE_BACK;
    fill_face_table(mn0, *res, face_base, *inv_leaf, table);
}

void voxel_general_plan(unsigned long n, int cus, int shrink, unsigned long *nwaves, unsigned long *per_wave) {
    *nwaves = general_plan_waves(n, cus, shrink);
    *per_wave = general_plan_per_wave(n, *nwaves);
}

void voxel_fast_plan(unsigned long n, int cus, int stagger, uint32_t out[4]) {
    const FastPlan p = fast_plan(n, cus, stagger);
    out[0] = p.blocks; out[1] = p.per_wg; out[2] = p.base_q; out[3] = p.inc_q;
}

// range_first_step(b) for b = 0 .. count - 1
void voxel_range_first_steps(uint32_t count, uint32_t base_q, uint32_t inc_q, uint32_t *out) {
    for (uint32_t b = 0; b < count; b++) out[b] = range_first_step(b, base_q, inc_q);
}

}
