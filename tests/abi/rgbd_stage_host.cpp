// rgbd_stage_host.cpp -- the RGB-D source's host staging (csrc/rgbd_stage.hpp: the rig's block, the aligned frame's block, the temporal
// state's block, a frame's upload sizes, the refusals of cameras, sensors, rigs and frames, a grab's plan) as a stand-alone host program
// for tests/test_rgbd_stage_host.py (built with -fsanitize=address,undefined: every block is on the heap and exactly as long as the
// header says, so a carve that leaves it ends the program).
//   rgbd_stage_host CHECK      one of the checks below; prints what does not hold and returns 1, else prints "ok" and returns 0
#include "rgbd_stage.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace cwipc_amd;

namespace {

int failures = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("line %d: %s does not hold\n", __LINE__, #cond);     \
            failures++;                                                 \
        }                                                               \
    } while (0)
#define EXPECT_TEXT(got, want)                                                                      \
    do {                                                                                            \
        const std::string got_ = (got), want_ = (want);                                             \
        if (got_ != want_) {                                                                        \
            printf("line %d: \"%s\" is not \"%s\"\n", __LINE__, got_.c_str(), want_.c_str());       \
            failures++;                                                                             \
        }                                                                                           \
    } while (0)

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
const char *const TOO_MANY = "more than 2^31 - 1 pixels";

size_t r256(size_t n) { return (n + 255) / 256 * 256; }   // (the test's own: not the header's)

cwipc_hip_rgbd_sensor sensor(int w, int h, int cw, int ch, int bpp, bool rational) {
    cwipc_hip_rgbd_sensor s;
    memset(&s, 0, sizeof(s));
    s.width = w; s.height = h; s.fx = 0.9 * w; s.fy = 1.1 * w; s.cx = 0.48 * w; s.cy = 0.53 * h;
    if (rational) { s.coeffs[0] = 0.1; s.coeffs[5] = 0.01; }
    s.depth_scale = 0.001;
    s.colour_width = cw; s.colour_height = ch; s.colour_bpp = bpp;
    s.colour_fx = 0.8 * cw; s.colour_fy = 0.9 * cw; s.colour_cx = 0.5 * cw; s.colour_cy = 0.5 * ch;
    for (int i = 0; i < 4; i++) s.depth_to_colour[5 * i] = s.trafo[5 * i] = 1.0;
    s.tile = 1;
    return s;
}

uint16_t a_depth_image[1];
uint8_t a_colour_image[16];
cwipc_hip_rgbd_camera camera(int w, int h, int bpp) {
    cwipc_hip_rgbd_camera c;
    memset(&c, 0, sizeof(c));
    c.width = w; c.height = h; c.bpp = bpp; c.depth = a_depth_image; c.colour = a_colour_image;   // (never read: the checks look at no image)
    c.fx = 0.9 * w; c.fy = 1.1 * w; c.cx = 0.48 * w; c.cy = 0.53 * h; c.depth_scale = 0.001;
    for (int i = 0; i < 4; i++) c.trafo[5 * i] = 1.0;
    c.tile = 1; c.serial = "cam";
    return c;
}

struct Region { std::string name; size_t at, bytes; };

// every region inside [0, total) and on a 256-byte boundary, no two overlapping; then every one written to its full extent in a heap
// block of exactly `total` bytes
void expect_regions(const std::vector<Region> &regions, size_t total) {
    for (size_t i = 0; i < regions.size(); i++) {
        const Region &r = regions[i];
        if (r.at + r.bytes > total || r.at % 256) { printf("region %s: [%zu, +%zu) of %zu\n", r.name.c_str(), r.at, r.bytes, total); failures++; return; }
        for (size_t j = i + 1; j < regions.size(); j++) {
            const Region &o = regions[j];
            if (r.at < o.at + o.bytes && o.at < r.at + r.bytes) { printf("regions %s and %s overlap\n", r.name.c_str(), o.name.c_str()); failures++; }
        }
    }
    uint8_t *block = (uint8_t *)malloc(total);   // (exactly the block: the sanitizer watches)
    if (!block) { EXPECT(!"memory"); return; }
    for (const Region &r : regions) memset(block + r.at, 0xa5, r.bytes);
    free(block);
}

struct Size { int w, h; };
const Size DEPTH_SIZES[] = {{1, 1}, {8, 8}, {63, 5}, {64, 64}, {65, 66}, {67, 45}, {513, 3}, {1280, 720}};
const Size COLOUR_SIZES[] = {{1, 1}, {33, 21}, {64, 48}, {101, 77}, {1920, 1080}};

uint32_t lcg_state = 12345;
uint32_t lcg() { return (lcg_state = lcg_state * 1664525u + 1013904223u) >> 8; }

// The block's bytes by the formula of rig_create before the size and the carve became one function.
size_t rig_bytes_before(const std::vector<cwipc_hip_rgbd_sensor> &grid, const std::vector<cwipc_hip_rgbd_sensor> &full, int decimation) {
    size_t bytes = r256(grid.size() * sizeof(k::RgbdRawCamDev));
    uint64_t total_words = 0;
    for (size_t k = 0; k < grid.size(); k++) {
        const cwipc_hip_rgbd_sensor &s = grid[k];
        const size_t npix = (size_t)s.width * (size_t)s.height, ncol = (size_t)s.colour_width * (size_t)s.colour_height;
        bool pinhole = true;
        for (int i = 0; i < 8; i++) pinhole = pinhole && s.coeffs[i] == 0.0;
        if (!pinhole) bytes += r256(npix * 16);
        bytes += r256(npix * 2) + r256(ncol * (size_t)s.colour_bpp + 8) + r256(npix * 3 + 8);
        if (decimation > 1) bytes += r256((size_t)full[k].width * (size_t)full[k].height * 2);
        total_words += (uint64_t)s.height * (((uint64_t)s.width + 63) / 64);
    }
    return bytes + r256((size_t)total_words * 8);
}

void expect_rig(const std::vector<cwipc_hip_rgbd_sensor> &full, int decimation) {
    const int ncam = (int)full.size();
    EXPECT_TEXT(rgbd_rig_refusal(full.data(), ncam, decimation), "");
    std::vector<cwipc_hip_rgbd_sensor> grid;
    for (const cwipc_hip_rgbd_sensor &s : full) grid.push_back(rgbd_grid_sensor(s, decimation));
    const RgbdRigLayout l = rgbd_rig_layout(grid.data(), full.data(), ncam, decimation);
    EXPECT(l.cams.size() == full.size() && l.table_bytes == r256((size_t)ncam * sizeof(k::RgbdRawCamDev)));
    std::vector<Region> regions = {{"table", 0, (size_t)ncam * sizeof(k::RgbdRawCamDev)}};
    uint32_t first = 0, wfirst = 0;
    size_t zfirst = 0;
    for (int k = 0; k < ncam; k++) {
        const cwipc_hip_rgbd_sensor &s = grid[(size_t)k], &whole = full[(size_t)k];
        const RgbdRigLayout::Cam &c = l.cams[(size_t)k];
        const std::string cam = "camera " + std::to_string(k) + " ";
        EXPECT(s.width == whole.width / decimation && s.height == whole.height / decimation && s.colour_width == whole.colour_width);
        const size_t npix = (size_t)s.width * (size_t)s.height, ncol = (size_t)s.colour_width * (size_t)s.colour_height;
        EXPECT((c.rays == 0) == (whole.coeffs[0] == 0.0) && (c.full_depth == 0) == (decimation == 1));
        EXPECT(c.depth != 0 && c.raw_colour != 0 && c.registered != 0);
        if (c.rays) regions.push_back({cam + "rays", c.rays, npix * 16});
        regions.push_back({cam + "depth", c.depth, npix * 2});
        regions.push_back({cam + "raw colour", c.raw_colour, ncol * (size_t)s.colour_bpp + 8});
        regions.push_back({cam + "registered", c.registered, npix * 3 + 8});
        const size_t full_bytes = (size_t)whole.width * (size_t)whole.height * 2;
        if (c.full_depth) regions.push_back({cam + "full depth", c.full_depth, (full_bytes + 15) / 16 * 16});
        EXPECT(c.first == first && c.wfirst == wfirst && c.zfirst == zfirst && c.wpr == (uint32_t)((s.width + 63) / 64));
        first += (uint32_t)npix;
        wfirst += (uint32_t)s.height * c.wpr;
        zfirst += ncol;
        // what a grab uploads of this camera, stated once for the staging size and the copies
        const RgbdFrameBytes b = rgbd_frame_bytes(whole);
        EXPECT(b.depth == full_bytes && b.colour == ncol * (size_t)whole.colour_bpp);
    }
    regions.push_back({"words", l.words, (size_t)wfirst * 8});
    EXPECT(l.total == first && l.total_words == wfirst && l.zwords == zfirst);
    EXPECT(l.bytes == rig_bytes_before(grid, full, decimation));
    expect_regions(regions, l.bytes);
}

void rig_block_layout() {
    for (int ncam = 1; ncam <= 4; ncam++)
        for (int decimation = 1; decimation <= 8; decimation++)
            for (int trial = 0; trial < 8; trial++) {
                std::vector<cwipc_hip_rgbd_sensor> full;
                for (int j = 0; j < ncam; j++) {
                    // camera 0 goes through the depth sizes in turn, the others take any; a size the decimation does not allow gives way
                    // to the next that it does
                    size_t pick = j == 0 ? (size_t)trial : lcg() % 8;
                    while (DEPTH_SIZES[pick].w < decimation || DEPTH_SIZES[pick].h < decimation) pick = (pick + 1) % 8;
                    const Size d = DEPTH_SIZES[pick];
                    const uint32_t r = lcg();
                    const Size c = r % 3 == 0 ? d : COLOUR_SIZES[(r >> 4) % 5];
                    full.push_back(sensor(d.w, d.h, c.w, c.h, 3 + (int)((r >> 8) & 1), ((r >> 9) & 1) != 0));
                }
                if (ncam > 1) {   // both lenses and both pixel sizes in every rig of more than one camera
                    full[0] = sensor(full[0].width, full[0].height, full[0].colour_width, full[0].colour_height, 3, true);
                    full[1] = sensor(full[1].width, full[1].height, full[1].colour_width, full[1].colour_height, 4, false);
                }
                expect_rig(full, decimation);
            }
    // the rig of the GPU test: every kind of part at odd sizes
    expect_rig({sensor(67, 45, 33, 21, 3, true), sensor(130, 9, 64, 48, 4, false)}, 2);
    // colour images of the depth image's size, and of one pixel, on every depth size
    for (const Size d : DEPTH_SIZES) {
        expect_rig({sensor(d.w, d.h, d.w, d.h, 3, true), sensor(d.w, d.h, 1, 1, 4, false)}, 1);
        expect_rig({sensor(d.w, d.h, d.w, d.h, 4, false)}, d.w >= 3 && d.h >= 3 ? 3 : 1);
    }
}

void frame_block_layout() {
    for (int ncam = 1; ncam <= 4; ncam++)
        for (int trial = 0; trial < 16; trial++) {
            std::vector<cwipc_hip_rgbd_camera> cams;
            for (int j = 0; j < ncam; j++) {
                const Size d = DEPTH_SIZES[j == 0 ? trial % 8 : lcg() % 8];
                cams.push_back(camera(d.w, d.h, j == 0 ? 3 + trial / 8 : 3 + (int)(lcg() & 1)));
            }
            EXPECT_TEXT(rgbd_frame_refusal(cams.data(), ncam, 3), "");
            const RgbdFrameLayout l = rgbd_frame_layout(cams.data(), ncam);
            EXPECT(l.cams.size() == cams.size() && l.table_bytes == r256((size_t)ncam * sizeof(k::RgbdCamDev)));
            std::vector<Region> regions = {{"table", 0, (size_t)ncam * sizeof(k::RgbdCamDev)}};
            size_t before = l.table_bytes;   // the parent commit's: round256(npix * 2) + round256(npix * bpp + 8) a camera
            uint32_t first = 0;
            for (int k = 0; k < ncam; k++) {
                const size_t npix = (size_t)cams[(size_t)k].width * (size_t)cams[(size_t)k].height, bpp = (size_t)cams[(size_t)k].bpp;
                const std::string cam = "camera " + std::to_string(k) + " ";
                regions.push_back({cam + "depth", l.cams[(size_t)k].depth, npix * 2});
                regions.push_back({cam + "colour", l.cams[(size_t)k].colour, npix * bpp + 8});   // (with the 8 readable bytes behind it)
                EXPECT(l.cams[(size_t)k].first == first);
                first += (uint32_t)npix;
                before += r256(npix * 2) + r256(npix * bpp + 8);
                const RgbdFrameBytes b = rgbd_frame_bytes(cams[(size_t)k]);
                EXPECT(b.depth == npix * 2 && b.colour == npix * bpp);
            }
            EXPECT(l.total == first && l.bytes == before);
            expect_regions(regions, l.bytes);
        }
}

void state_block_views() {
    const std::vector<std::vector<cwipc_hip_rgbd_sensor>> rigs = {
        {sensor(1, 1, 1, 1, 3, false)},
        {sensor(31, 1, 1, 1, 3, false), sensor(1, 1, 1, 1, 3, false)},
        {sensor(16, 16, 1, 1, 3, false)},
        {sensor(67, 45, 33, 21, 3, true), sensor(130, 9, 64, 48, 4, false), sensor(1, 1, 1, 1, 3, false), sensor(16, 2, 1, 1, 3, false)},
        {sensor(1280, 720, 8, 8, 3, false), sensor(513, 3, 8, 8, 3, false), sensor(1280, 720, 8, 8, 3, false)},
    };
    for (const auto &grid : rigs)
        for (int extra = 0; extra < 2; extra++) {   // (extra: the last camera's pixels counted one short of a 256-byte line's end and one past it)
            const RgbdRigLayout rig = rgbd_rig_layout(grid.data(), grid.data(), (int)grid.size(), 1);
            const uint32_t total = rig.total;
            const RgbdStateLayout l = rgbd_state_layout(total);
            EXPECT(l.history == r256((size_t)total * 8) && l.bytes == r256((size_t)total * 8) + total);   // the parent commit's formula
            EXPECT(l.history % 256 == 0 && l.history >= (size_t)total * 8);
            uint8_t *block = (uint8_t *)malloc(l.bytes);   // (exactly the block: the sanitizer watches)
            if (!block) { EXPECT(!"memory"); return; }
            memset(block, 0, l.bytes);                               // the clear: the whole block
            size_t value_end = 0, history_end = l.history;
            for (size_t k = 0; k < grid.size(); k++) {               // a camera's two views, as the grab's kernel and rig_history see them
                const size_t npix = (size_t)grid[k].width * (size_t)grid[k].height;
                EXPECT(l.value_at(rig.cams[k].first) == value_end && l.history_at(rig.cams[k].first) == history_end);
                memset(block + l.value_at(rig.cams[k].first), 0xa5, npix * 8);
                memset(block + l.history_at(rig.cams[k].first), 0x5a, npix);
                value_end += npix * 8;
                history_end += npix;
            }
            EXPECT(value_end == (size_t)total * 8 && value_end <= l.history && history_end == l.bytes);
            free(block);
        }
    for (uint32_t total : {1u, 31u, 32u, 33u, 255u, 256u, 257u, 0x7fffffffu}) {
        const RgbdStateLayout l = rgbd_state_layout(total);
        EXPECT(l.history == r256((size_t)total * 8) && l.bytes == l.history + total && l.value_at(total - 1) + 8 <= l.history && l.history_at(total - 1) < l.bytes);
    }
}

// 2^31 - 1 is prime: 32768 x 65535 and 32767 x 1 pixels are that many together
void pixel_limits() {
    std::vector<cwipc_hip_rgbd_camera> cams = {camera(32768, 65535, 3), camera(32767, 1, 4)};
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 0), "");
    const RgbdFrameLayout frame = rgbd_frame_layout(cams.data(), 2);   // (sizes alone: nothing is allocated)
    EXPECT(frame.total == 0x7fffffffu);
    EXPECT(frame.bytes == r256(2 * sizeof(k::RgbdCamDev)) + r256(2147450880ull * 2) + r256(2147450880ull * 3 + 8) + r256(32767 * 2) + r256(32767 * 4 + 8));
    cams[1].width = 32768;
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 0), TOO_MANY);
    cams[1] = camera(0x7fffffff, 0x7fffffff, 3);   // (the sum does not wrap)
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 0), TOO_MANY);
    cams.push_back(camera(0x7fffffff, 0x7fffffff, 3));
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 3, 0), TOO_MANY);
    cams[0] = camera(0x7fffffff, 1, 3);
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 1, 0), "");
    cams[0] = camera(0x7fffffff, 2, 3);
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 1, 0), TOO_MANY);

    // a rig counts the full-size depth images, whatever the decimation, and every colour image on its own.  Decimated by 8 no image
    // is lower than 8 rows: 32768 x 65528 and 29127 x 9 are 2^31 - 1 pixels, 32768 x 65528 and 32768 x 8 are 2^31
    const struct { int decimation; Size first, last, one_more; } rigs[] = {{1, {32768, 65535}, {32767, 1}, {32768, 1}}, {8, {32768, 65528}, {29127, 9}, {32768, 8}}};
    for (const auto &r : rigs) {
        std::vector<cwipc_hip_rgbd_sensor> sensors = {sensor(r.first.w, r.first.h, 1, 1, 3, false), sensor(r.last.w, r.last.h, 1, 1, 4, true)};
        EXPECT((uint64_t)r.first.w * r.first.h + (uint64_t)r.last.w * r.last.h == 0x7fffffffull);
        EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, r.decimation), "");
        const std::vector<cwipc_hip_rgbd_sensor> grid = {rgbd_grid_sensor(sensors[0], r.decimation), rgbd_grid_sensor(sensors[1], r.decimation)};
        const RgbdRigLayout l = rgbd_rig_layout(grid.data(), sensors.data(), 2, r.decimation);   // (sizes alone: nothing is allocated)
        EXPECT(l.total == (uint32_t)(r.first.w / r.decimation) * (uint32_t)(r.first.h / r.decimation) + (uint32_t)(r.last.w / r.decimation) * (uint32_t)(r.last.h / r.decimation));
        EXPECT(l.zwords == 2 && l.cams[1].first == (uint32_t)(r.first.w / r.decimation) * (uint32_t)(r.first.h / r.decimation));
        sensors[1] = sensor(r.one_more.w, r.one_more.h, 1, 1, 4, true);
        EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, r.decimation), TOO_MANY);
    }
    cwipc_hip_rgbd_sensor s = sensor(8, 8, 46340, 46340, 3, false);
    EXPECT_TEXT(rgbd_rig_refusal(&s, 1, 1), "");
    s.colour_width = 65536; s.colour_height = 32768;
    EXPECT_TEXT(rgbd_rig_refusal(&s, 1, 1), std::string("camera 0: ") + TOO_MANY);
    s.colour_width = 0x7fffffff; s.colour_height = 1;
    EXPECT_TEXT(rgbd_rig_refusal(&s, 1, 1), "");
}

void camera_refusals() {
    const cwipc_hip_rgbd_camera good = camera(67, 45, 3);
    EXPECT(rgbd_camera_problem(good) == nullptr);
    const auto problem = [&](void (*spoil)(cwipc_hip_rgbd_camera &)) { cwipc_hip_rgbd_camera c = good; spoil(c); const char *p = rgbd_camera_problem(c); return std::string(p ? p : ""); };
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.width = 0; }), "width and height must be at least 1");
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.height = -3; }), "width and height must be at least 1");
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.bpp = 2; }), "bpp must be 3 (R, G, B) or 4 (B, G, R, A)");
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.bpp = 5; }), "bpp must be 3 (R, G, B) or 4 (B, G, R, A)");
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.cx = NaN; }), "the intrinsics, depth_scale and the matrix must be finite");
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.depth_scale = INF; }), "the intrinsics, depth_scale and the matrix must be finite");
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.trafo[15] = NaN; }), "the intrinsics, depth_scale and the matrix must be finite");
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.fx = 0.0; }), "fx and fy must not be zero");
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.fy = -0.0; }), "fx and fy must not be zero");
    // in the order they are tested: size, bpp, finite, focal lengths
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.width = 0; c.bpp = 7; c.fx = NaN; }), "width and height must be at least 1");
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.bpp = 7; c.fx = NaN; c.fy = 0.0; }), "bpp must be 3 (R, G, B) or 4 (B, G, R, A)");
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_camera &c) { c.fx = NaN; c.fy = 0.0; }), "the intrinsics, depth_scale and the matrix must be finite");

    // the frame: NULL, ncam, then camera after camera its pointers, its numbers, the pixels so far
    std::vector<cwipc_hip_rgbd_camera> cams = {good, camera(64, 48, 4)};
    EXPECT_TEXT(rgbd_frame_refusal(nullptr, 2, 0), "NULL argument");
    EXPECT_TEXT(rgbd_frame_refusal(nullptr, 0, 0), "NULL argument");
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 0, 0), "ncam must be at least 1");
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), -1, 0), "ncam must be at least 1");
    cams[1].depth = nullptr;
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 0), "camera 1: NULL argument");
    cams[1] = camera(64, 48, 4); cams[1].colour = nullptr; cams[1].bpp = 9;
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 0), "camera 1: NULL argument");
    cams[1] = camera(64, 48, 4); cams[1].serial = nullptr;
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 0), "");                           // (no serial is needed when nothing is attached)
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 1), "camera 1: NULL argument");
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 2), "camera 1: NULL argument");
    cams[0].bpp = 5;
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 2), "camera 0: bpp must be 3 (R, G, B) or 4 (B, G, R, A)");   // (camera 0 is looked at first)
    cams[0] = good; cams[1] = camera(64, 48, 4); cams[1].fx = 0.0;
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 0), "camera 1: fx and fy must not be zero");
    cams[0] = camera(0x7fffffff, 2, 3);
    EXPECT_TEXT(rgbd_frame_refusal(cams.data(), 2, 0), TOO_MANY);                    // (the pixels so far come before the next camera)
}

void sensor_refusals() {
    const cwipc_hip_rgbd_sensor good = sensor(67, 45, 33, 21, 3, true);
    EXPECT(rgbd_sensor_problem(good) == nullptr);
    const auto problem = [&](void (*spoil)(cwipc_hip_rgbd_sensor &)) { cwipc_hip_rgbd_sensor s = good; spoil(s); const char *p = rgbd_sensor_problem(s); return std::string(p ? p : ""); };
    const char *const SIZE = "width and height must be at least 1", *const BPP = "colour_bpp must be 3 (R, G, B) or 4 (B, G, R, A)",
                      *const FINITE = "the intrinsics, the lens coefficients, depth_scale and the matrices must be finite", *const FOCAL = "fx and fy must not be zero";
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.width = 0; }), SIZE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.height = 0; }), SIZE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_width = 0; }), SIZE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_height = -1; }), SIZE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_width = 65536; s.colour_height = 32768; }), TOO_MANY);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_bpp = 5; }), BPP);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_bpp = 0; }), BPP);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.cy = NaN; }), FINITE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_cx = INF; }), FINITE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.coeffs[7] = NaN; }), FINITE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_coeffs[0] = -INF; }), FINITE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.depth_to_colour[3] = NaN; }), FINITE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.trafo[12] = NaN; }), FINITE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.depth_scale = NaN; }), FINITE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.fx = 0.0; }), FOCAL);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.fy = 0.0; }), FOCAL);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_fx = 0.0; }), FOCAL);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_fy = 0.0; }), FOCAL);
    // in the order they are tested: sizes, colour pixels, bpp, finite, focal lengths
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.width = 0; s.colour_width = 65536; s.colour_height = 32768; s.colour_bpp = 5; }), SIZE);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_width = 65536; s.colour_height = 32768; s.colour_bpp = 5; s.fx = NaN; }), TOO_MANY);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.colour_bpp = 5; s.fx = NaN; s.fy = 0.0; }), BPP);
    EXPECT_TEXT(problem([](cwipc_hip_rgbd_sensor &s) { s.fx = NaN; s.fy = 0.0; }), FINITE);
}

void rig_refusals() {
    std::vector<cwipc_hip_rgbd_sensor> sensors = {sensor(67, 45, 33, 21, 3, true), sensor(9, 5, 8, 8, 4, false)};
    EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, 1), "");
    EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, 5), "");   // (5 is the second camera's height: a grid one pixel high)
    EXPECT_TEXT(rgbd_rig_refusal(nullptr, 2, 1), "NULL argument");
    EXPECT_TEXT(rgbd_rig_refusal(nullptr, 0, 0), "NULL argument");
    EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 0, 1), "ncam must be at least 1");
    EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), -2, 0), "ncam must be at least 1");
    for (int decimation : {0, -1, 9, 64}) EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, decimation), "decimation must be between 1 and 8");
    for (int decimation : {6, 8}) EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, decimation), "camera 1: width and height must be at least the decimation");
    sensors[1] = sensor(5, 9, 8, 8, 4, false);
    EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, 6), "camera 1: width and height must be at least the decimation");
    // the decimation before any sensor; a sensor's own problem before its size under the decimation; camera 0 before camera 1
    sensors[0].colour_bpp = 5;
    EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, 9), "decimation must be between 1 and 8");
    EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, 6), "camera 0: colour_bpp must be 3 (R, G, B) or 4 (B, G, R, A)");
    sensors[0] = sensor(67, 45, 33, 21, 3, true); sensors[1].fx = 0.0;
    EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, 6), "camera 1: fx and fy must not be zero");
    sensors[0] = sensor(0x7fffffff, 8, 1, 1, 3, false); sensors[1] = sensor(5, 9, 8, 8, 4, false);
    EXPECT_TEXT(rgbd_rig_refusal(sensors.data(), 2, 6), TOO_MANY);   // (camera 0's pixels come before camera 1 is looked at)
}

struct Options {
    cwipc_hip_rgbd_holefill holefill;
    cwipc_hip_rgbd_depthfilter depthfilter;
    cwipc_hip_rgbd_prep prep;
    cwipc_hip_rgbd_occlusion occlusion;
};
// every stage on, every number in order
Options all_on() {
    Options o;
    o.holefill.mode = 2;
    o.depthfilter.spatial_magnitude = 1; o.depthfilter.spatial_alpha = 0.5; o.depthfilter.spatial_delta = 20.0;
    o.depthfilter.temporal = 1; o.depthfilter.temporal_alpha = 0.4; o.depthfilter.temporal_delta = 30.0; o.depthfilter.temporal_persistency = 3;
    o.prep.depth_x_erosion = 1; o.prep.depth_y_erosion = 2;
    o.occlusion.splat = 1; o.occlusion.margin = 0.02;
    return o;
}
std::string plan_of(const Options &o, RgbdGrabPlan &plan) { return rgbd_grab_plan(&o.holefill, &o.depthfilter, &o.prep, &o.occlusion, plan); }

const char *const EROSION = "depth_x_erosion and depth_y_erosion must be between 0 and 32", *const SPLAT = "occlusion: splat must be between 0 and 8",
                  *const MARGIN = "occlusion: margin must be finite and not negative", *const MAGNITUDE = "depthfilter: spatial_magnitude must be between 0 and 5",
                  *const PERSISTENCY = "depthfilter: temporal_persistency must be between 0 and 8",
                  *const SPATIAL_ALPHA = "depthfilter: spatial_alpha must be greater than 0 and at most 1",
                  *const SPATIAL_DELTA = "depthfilter: spatial_delta must be finite and greater than 0",
                  *const TEMPORAL_ALPHA = "depthfilter: temporal_alpha must be greater than 0 and at most 1",
                  *const TEMPORAL_DELTA = "depthfilter: temporal_delta must be finite and greater than 0", *const MODE = "holefill: mode must be between 0 and 3";

bool same_terms(const RgbdSmoothTerms &a, const RgbdSmoothTerms &b) { return memcmp(&a.alpha, &b.alpha, 8) == 0 && memcmp(&a.oma, &b.oma, 8) == 0 && memcmp(&a.delta, &b.delta, 8) == 0; }
bool same_plan(const RgbdGrabPlan &a, const RgbdGrabPlan &b) {
    return a.ex == b.ex && a.ey == b.ey && a.magnitude == b.magnitude && same_terms(a.spatial, b.spatial) && a.temporal == b.temporal &&
           same_terms(a.temporal_terms, b.temporal_terms) && a.persistency == b.persistency && a.fill_mode == b.fill_mode && a.occluded == b.occluded &&
           a.splat == b.splat && memcmp(&a.margin, &b.margin, 8) == 0;
}

void grab_plan_refusals() {
    RgbdGrabPlan untouched;
    untouched.ex = 77;
    const auto refusal = [&](void (*spoil)(Options &)) { Options o = all_on(); spoil(o); const std::string text = plan_of(o, untouched); EXPECT(text.empty() || untouched.ex == 77); untouched.ex = 77; return text; };   // (a refusal sets no plan)
    EXPECT_TEXT(refusal([](Options &o) { o.prep.depth_x_erosion = -1; }), EROSION);
    EXPECT_TEXT(refusal([](Options &o) { o.prep.depth_x_erosion = 33; }), EROSION);
    EXPECT_TEXT(refusal([](Options &o) { o.prep.depth_y_erosion = -1; }), EROSION);
    EXPECT_TEXT(refusal([](Options &o) { o.prep.depth_y_erosion = 33; }), EROSION);
    EXPECT_TEXT(refusal([](Options &o) { o.occlusion.splat = -1; }), SPLAT);
    EXPECT_TEXT(refusal([](Options &o) { o.occlusion.splat = 9; }), SPLAT);
    EXPECT_TEXT(refusal([](Options &o) { o.occlusion.margin = -1e-9; }), MARGIN);
    EXPECT_TEXT(refusal([](Options &o) { o.occlusion.margin = NaN; }), MARGIN);
    EXPECT_TEXT(refusal([](Options &o) { o.occlusion.margin = INF; }), MARGIN);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_magnitude = -1; }), MAGNITUDE);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_magnitude = 6; }), MAGNITUDE);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.temporal_persistency = -1; }), PERSISTENCY);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.temporal_persistency = 9; }), PERSISTENCY);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_alpha = 0.0; }), SPATIAL_ALPHA);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_alpha = 1.0000001; }), SPATIAL_ALPHA);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_alpha = NaN; }), SPATIAL_ALPHA);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_delta = 0.0; }), SPATIAL_DELTA);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_delta = INF; }), SPATIAL_DELTA);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_delta = NaN; }), SPATIAL_DELTA);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.temporal_alpha = -0.5; }), TEMPORAL_ALPHA);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.temporal_alpha = 2.0; }), TEMPORAL_ALPHA);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.temporal_alpha = INF; }), TEMPORAL_ALPHA);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.temporal_delta = -1.0; }), TEMPORAL_DELTA);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.temporal_delta = NaN; }), TEMPORAL_DELTA);
    for (int mode : {-1, 4, 99}) {
        Options o = all_on();
        o.holefill.mode = mode;
        EXPECT_TEXT(plan_of(o, untouched), MODE);
    }
    // the ends of every range are inside it
    EXPECT_TEXT(refusal([](Options &o) { o.prep.depth_x_erosion = 32; o.prep.depth_y_erosion = 0; o.occlusion.splat = 8; o.occlusion.margin = 0.0; }), "");
    EXPECT_TEXT(refusal([](Options &o) { o.occlusion.splat = 0; o.depthfilter.spatial_magnitude = 5; o.depthfilter.temporal_persistency = 8; o.holefill.mode = 3; }), "");
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_alpha = 1.0; o.depthfilter.temporal_alpha = 1.0; o.depthfilter.temporal_persistency = 0; }), "");
    // an alpha or a delta is not looked at when its stage is off; the persistency is
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_magnitude = 0; o.depthfilter.spatial_alpha = NaN; o.depthfilter.spatial_delta = -1.0; }), "");
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.temporal = 0; o.depthfilter.temporal_alpha = 7.0; o.depthfilter.temporal_delta = NaN; }), "");
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.temporal = 0; o.depthfilter.temporal_persistency = 9; }), PERSISTENCY);
    EXPECT_TEXT(refusal([](Options &o) { o.depthfilter.spatial_magnitude = 0; o.depthfilter.temporal = 0; o.depthfilter.temporal_persistency = -1; }), PERSISTENCY);
    untouched.ex = 77;

    // two options wrong at once: the one named first today is named first still
    const struct { void (*spoil)(Options &); const char *text; } wrong[] = {
        {[](Options &o) { o.prep.depth_y_erosion = 40; }, EROSION},
        {[](Options &o) { o.occlusion.splat = 9; }, SPLAT},
        {[](Options &o) { o.occlusion.margin = -1.0; }, MARGIN},
        {[](Options &o) { o.depthfilter.spatial_magnitude = 6; }, MAGNITUDE},
        {[](Options &o) { o.depthfilter.temporal_persistency = 9; }, PERSISTENCY},
        {[](Options &o) { o.depthfilter.spatial_alpha = 0.0; }, SPATIAL_ALPHA},
        {[](Options &o) { o.depthfilter.spatial_delta = 0.0; }, SPATIAL_DELTA},
        {[](Options &o) { o.depthfilter.temporal_alpha = 0.0; }, TEMPORAL_ALPHA},
        {[](Options &o) { o.depthfilter.temporal_delta = 0.0; }, TEMPORAL_DELTA},
        {[](Options &o) { o.holefill.mode = 4; }, MODE},
    };
    for (size_t i = 0; i < 10; i++)
        for (size_t j = i + 1; j < 10; j++) {
            Options o = all_on();
            wrong[j].spoil(o);
            wrong[i].spoil(o);
            RgbdGrabPlan plan;
            EXPECT_TEXT(plan_of(o, plan), wrong[i].text);
        }
}

void grab_plans() {
    const RgbdGrabPlan nothing;
    EXPECT(nothing.ex == 0 && nothing.ey == 0 && nothing.magnitude == 0 && !nothing.temporal && nothing.persistency == 0 && nothing.fill_mode == 0 && !nothing.occluded &&
           nothing.splat == 0 && nothing.margin == 0.0 && nothing.spatial.alpha == 0.0 && nothing.spatial.oma == 0.0 && nothing.spatial.delta == 0.0 &&
           nothing.temporal_terms.alpha == 0.0 && nothing.temporal_terms.oma == 0.0 && nothing.temporal_terms.delta == 0.0);
    // every stage on: every number arrives
    const Options on = all_on();
    RgbdGrabPlan plan;
    EXPECT_TEXT(plan_of(on, plan), "");
    EXPECT(plan.ex == 1 && plan.ey == 2 && plan.magnitude == 1 && plan.temporal && plan.persistency == 3 && plan.fill_mode == 2 && plan.occluded && plan.splat == 1 &&
           plan.margin == 0.02);
    EXPECT(same_terms(plan.spatial, rgbd_smooth_terms(0.5, 20.0)) && same_terms(plan.temporal_terms, rgbd_smooth_terms(0.4, 30.0)) && plan.temporal_terms.oma == 1.0 - 0.4);
    // all four structs NULL: the plain grab without erosion, which does nothing but register, count and scatter
    RgbdGrabPlan none;
    none.ex = 5;
    EXPECT_TEXT(rgbd_grab_plan(nullptr, nullptr, nullptr, nullptr, none), "");
    EXPECT(same_plan(none, nothing));
    // the plain grab (prep alone) and the occluded grab (prep and occlusion), through the entries that take more: a holefill of
    // mode 0 and a depthfilter with both stages off -- whatever else it holds -- give the same plan as NULL
    for (const cwipc_hip_rgbd_occlusion *occlusion : {(const cwipc_hip_rgbd_occlusion *)nullptr, &on.occlusion})
        for (const cwipc_hip_rgbd_prep *prep : {(const cwipc_hip_rgbd_prep *)nullptr, &on.prep}) {
            RgbdGrabPlan plain, filtered, filled;
            EXPECT_TEXT(rgbd_grab_plan(nullptr, nullptr, prep, occlusion, plain), "");
            EXPECT(plain.ex == (prep ? 1 : 0) && plain.ey == (prep ? 2 : 0) && plain.occluded == (occlusion != nullptr) && plain.splat == (occlusion ? 1 : 0));
            EXPECT(plain.magnitude == 0 && !plain.temporal && plain.fill_mode == 0);
            cwipc_hip_rgbd_depthfilter off = on.depthfilter;
            off.spatial_magnitude = 0; off.temporal = 0;
            off.spatial_alpha = NaN; off.temporal_delta = -3.0; off.temporal_persistency = 8;
            cwipc_hip_rgbd_holefill no_fill;
            no_fill.mode = 0;
            EXPECT_TEXT(rgbd_grab_plan(nullptr, &off, prep, occlusion, filtered), "");
            EXPECT_TEXT(rgbd_grab_plan(&no_fill, &off, prep, occlusion, filled), "");
            EXPECT(same_plan(filtered, plain) && same_plan(filled, plain));
            EXPECT_TEXT(rgbd_grab_plan(&no_fill, nullptr, prep, occlusion, filled), "");
            EXPECT(same_plan(filled, plain));
        }
    // one stage on leaves the other's numbers 0
    Options spatial_only = all_on();
    spatial_only.depthfilter.temporal = 0;
    EXPECT_TEXT(plan_of(spatial_only, plan), "");
    EXPECT(plan.magnitude == 1 && !plan.temporal && plan.persistency == 0 && same_terms(plan.temporal_terms, nothing.temporal_terms));
    Options temporal_only = all_on();
    temporal_only.depthfilter.spatial_magnitude = 0;
    EXPECT_TEXT(plan_of(temporal_only, plan), "");
    EXPECT(plan.magnitude == 0 && plan.temporal && plan.persistency == 3 && same_terms(plan.spatial, nothing.spatial));
}

const struct { const char *name; void (*run)(); } CHECKS[] = {
    {"rig_block_layout", rig_block_layout},
    {"frame_block_layout", frame_block_layout},
    {"state_block_views", state_block_views},
    {"pixel_limits", pixel_limits},
    {"camera_refusals", camera_refusals},
    {"sensor_refusals", sensor_refusals},
    {"rig_refusals", rig_refusals},
    {"grab_plan_refusals", grab_plan_refusals},
    {"grab_plans", grab_plans},
};

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2)
        for (const auto &check : CHECKS)
            if (strcmp(argv[1], check.name) == 0) {
                check.run();
                if (failures == 0) printf("ok\n");
                return failures ? 1 : 0;
            }
    fprintf(stderr, "usage: rgbd_stage_host CHECK, one of:\n");
    for (const auto &check : CHECKS) fprintf(stderr, "  %s\n", check.name);
    return 2;
}
