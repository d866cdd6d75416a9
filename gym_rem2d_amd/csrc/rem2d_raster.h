// rem2d_raster.h -- the creature renderer (include/rem2d_render.h): uint8 RGB frames [K][H][W][3] of K creatures of one world,
// read from the state arena and the uploaded terrain in place.
// Part of the single translation unit rem2d.hip (see its header comment); not a stand-alone header.
//
// The scene is the one Modular2DEnv.render draws (gym_rem2D/envs/Modular2DEnv.py:655-738), in its painter order: sky, ground
// fill under every terrain edge down to y = 0, the terrain edges as 2-px lines, the hardcore obstacles (fill + 2-px outline),
// the creature's bodies in slot order (box: filled quad + 2-px outline; circle: filled disc + 2-px ring), the wall of death
// (1-px line, y in [-10, 40]) and the flag.  Clouds, DISPLAY_VECTORS / DISPLAY_JOINTS and COLOR_CONTROL are not drawn.
//
// Every pixel is defined exactly, so that a CPU model (tests/render_model.py) matches it with ==:
//   * pixel (i, j) has its centre at X = cam_x + (i + 0.5) * INV_SCALE, Y = (cam_y + H * INV_SCALE) - (j + 0.5) * INV_SCALE;
//   * coverage uses + - * and comparisons only, every operation a separately rounded binary32 one in every build.  The
//     __fmul_rn / __fadd_rn spelling does not give that by itself (they are the plain operators here, and -ffp-contract=fast
//     fuses a product into the sum that consumes it: librem2d_fma.so drew other pixels until every product that a sum
//     takes went through sn_keep(), rem2d_math.h -- r_mul; r_sq is the lone product; tests/test_render_forge_gpu.py compares the three builds): edge functions
//     cross(b - a, p - a) for quads, the triangle and the ground,
//     d^2 <= r^2 for discs, (r - h)^2 < d^2 <= (r + h)^2 for rings, and for a line band of half width h along a -> b
//     cross^2 <= h^2 * |b - a|^2 with 0 <= dot(b - a, p - a) <= |b - a|^2 (butt ends);
//   * a body's rotation is the engine's own rot_set(angle).
#ifndef REM2D_RASTER_H
#define REM2D_RASTER_H

// colours: round(255 * c) of the reference's float colours (Python's round, half to even)
#define RGB(r, g, b) ((unsigned)(r) | ((unsigned)(g) << 8) | ((unsigned)(b) << 16))
constexpr unsigned RC_SKY = RGB(230, 230, 255);       // (0.9, 0.9, 1.0)
constexpr unsigned RC_GROUND = RGB(102, 153, 76);     // (0.4, 0.6, 0.3)
constexpr unsigned RC_EDGE_EVEN = RGB(76, 255, 76);   // (0.3, 1.0, 0.3): edge i, i even
constexpr unsigned RC_EDGE_ODD = RGB(76, 204, 76);    // (0.3, 0.8, 0.3): edge i, i odd
constexpr unsigned RC_OBST_FILL = RGB(255, 255, 255); // (1, 1, 1)
constexpr unsigned RC_OBST_LINE = RGB(153, 153, 153); // (0.6, 0.6, 0.6)
constexpr unsigned RC_WOD = RGB(0, 0, 255);           // (0, 0, 1)
constexpr unsigned RC_FLAG_LINE = RGB(0, 0, 0);       // (0, 0, 0): pole and outline
constexpr unsigned RC_FLAG_FILL = RGB(230, 51, 0);    // (0.9, 0.2, 0)
// bodies without a colour table (rem2d_world_render with NULL tables): one colour pair per shape
constexpr unsigned RC_BOX_FILL = RGB(127, 166, 217), RC_BOX_LINE = RGB(31, 63, 102);
constexpr unsigned RC_CIRCLE_FILL = RGB(217, 166, 127), RC_CIRCLE_LINE = RGB(102, 64, 31);
#undef RGB

constexpr float R_INV_SCALE = (float)(1.0 / 30.0); // 1 / SCALE, rounded once
constexpr float R_HALF_PX = 0.5f * R_INV_SCALE;     // (exact)
// the flag (Modular2DEnv.py:730-737): pole (FX, FY1) -> (FX, FY2), triangle (FX, FY2), (FX, FY3), (FX2, FY4) -- counter-clockwise
constexpr float R_FLAG_X = (float)(14.0 / 30.0 * 3.0);                 // TERRAIN_STEP * 3
constexpr float R_FLAG_Y1 = (float)(600.0 / 30.0 / 4.0);               // TERRAIN_HEIGHT
constexpr float R_FLAG_Y2 = (float)(600.0 / 30.0 / 4.0 + 50.0 / 30.0); // + 50 / SCALE
constexpr float R_FLAG_Y3 = (float)(600.0 / 30.0 / 4.0 + 50.0 / 30.0 - 10.0 / 30.0);
constexpr float R_FLAG_X2 = (float)(14.0 / 30.0 * 3.0 + 25.0 / 30.0);
constexpr float R_FLAG_Y4 = (float)(600.0 / 30.0 / 4.0 + 50.0 / 30.0 - 5.0 / 30.0);
constexpr float R_WOD_Y0 = -10.0f, R_WOD_Y1 = 40.0f;

// launch shape: a 256-thread workgroup covers a 64 x 16 pixel tile of one image; lane t draws the 4 horizontally adjacent
// pixels (4 (t % 16), t / 16) of it and stores their 12 bytes with three dword stores (a wave writes 4 rows of 192 bytes)
constexpr int R_TILE_W = 64, R_TILE_H = 16, R_PX_PER_LANE = 4, R_THREADS = 256;
constexpr int R_MAX_SIZE = 8192; // largest width / height rem2d_world_render takes
constexpr int R_MAX_TILE_OBST = 64; // obstacles listed per tile (more: every pixel of the tile tests all of them)

// one body of the creature, in world space (LDS): a box's four CCW edges a -> a + d with |d|^2 and h^2 |d|^2, or a circle's
// centre and squared radii
struct RBody {
    float ax[4], ay[4], dx[4], dy[4], len2[4], hh[4];
    float lx, ly, ux, uy; // bounding box (for the per-tile cull)
    int shape;
    unsigned fill, line;
};

DEV float r_add(float a, float b) { return __fadd_rn(a, b); }
DEV float r_sub(float a, float b) { return __fsub_rn(a, b); }
DEV float r_mul(float a, float b) { return sn_keep(__fmul_rn(a, b)); } // a product that a sum takes: kept, so that it cannot fuse into it
DEV float r_sq(float a, float b) { return __fmul_rn(a, b); }           // a product that only a comparison (or a store) takes: nothing to fuse with
// cross(d, p - a) and dot(d, p - a)
DEV void r_edge(float ax, float ay, float dx, float dy, float X, float Y, float &cr, float &dt) {
    const float qx = r_sub(X, ax), qy = r_sub(Y, ay);
    cr = r_sub(r_mul(dx, qy), r_mul(dy, qx));
    dt = r_add(r_mul(dx, qx), r_mul(dy, qy));
}
DEV bool r_band(float cr, float dt, float len2, float hh) { return r_sq(cr, cr) <= hh && dt >= 0.0f && dt <= len2; }
// a segment a -> b as a band of half width 1 px
DEV bool r_segment(float ax, float ay, float bx, float by, float X, float Y) {
    const float dx = r_sub(bx, ax), dy = r_sub(by, ay);
    const float len2 = r_add(r_mul(dx, dx), r_mul(dy, dy));
    float cr, dt;
    r_edge(ax, ay, dx, dy, X, Y, cr, dt);
    return r_band(cr, dt, len2, r_sq(r_sq(R_INV_SCALE, R_INV_SCALE), len2));
}
// the colour of a convex quad / triangle (CCW vertices) over `c`: fill where every edge function is >= 0, then the outline
DEV unsigned r_poly(const float *vx, const float *vy, int n, float X, float Y, unsigned fill, unsigned line, unsigned c) {
    bool inside = true, edge = false;
    for (int k = 0; k < n; ++k) {
        const int k1 = k + 1 == n ? 0 : k + 1;
        const float dx = r_sub(vx[k1], vx[k]), dy = r_sub(vy[k1], vy[k]);
        const float len2 = r_add(r_mul(dx, dx), r_mul(dy, dy));
        float cr, dt;
        r_edge(vx[k], vy[k], dx, dy, X, Y, cr, dt);
        inside = inside && cr >= 0.0f;
        edge = edge || r_band(cr, dt, len2, r_sq(r_sq(R_INV_SCALE, R_INV_SCALE), len2));
    }
    return edge ? line : (inside ? fill : c);
}

DEV unsigned r_shade(float X, float Y, const Terrain &T, const RBody *bodies, const int *list, int nList, const int *obst, int nObst,
                     float wod) {
    unsigned c = RC_SKY;
    // terrain edges near X: the edge index from the (uniform) pitch, +-1 for the +-0.1 pitch the xs may deviate by
    float fi = r_sq(r_sub(X, T.x0), T.invPitch);
    fi = fi < -2.0f ? -2.0f : (fi > (float)T.nEdge + 1.0f ? (float)T.nEdge + 1.0f : fi);
    const int i0 = (int)floorf(fi);
    // ground: below edge i (cross(b - a, p - a) <= 0), x between its ends, y >= 0
    for (int i = i0 - 1; i <= i0 + 1; ++i) {
        if (i < 0 || i >= T.nEdge) continue;
        const int s = T.nPoly + i;
        const float ax = T.vx[s], ay = T.vy[s], bx = T.vx[T.nStatic + s], by = T.vy[T.nStatic + s];
        float cr, dt;
        r_edge(ax, ay, r_sub(bx, ax), r_sub(by, ay), X, Y, cr, dt);
        if (X >= ax && X <= bx && Y >= 0.0f && cr <= 0.0f) c = RC_GROUND;
    }
    // edge lines, drawn last edge first (the reference's drawlist is the terrain list reversed): the lowest index wins
    for (int i = i0 + 1; i >= i0 - 1; --i) {
        if (i < 0 || i >= T.nEdge) continue;
        const int s = T.nPoly + i;
        if (r_segment(T.vx[s], T.vy[s], T.vx[T.nStatic + s], T.vy[T.nStatic + s], X, Y)) c = (i & 1) ? RC_EDGE_ODD : RC_EDGE_EVEN;
    }
    // obstacles (this tile's, in drawing order: last created first; nObst < 0: more than the list holds, all of them)
    const int nO = nObst < 0 ? T.nPoly : nObst;
    for (int k = 0; k < nO; ++k) {
        const int s = nObst < 0 ? T.nPoly - 1 - k : obst[k];
        const float vx[4] = {T.vx[s], T.vx[T.nStatic + s], T.vx[2 * T.nStatic + s], T.vx[3 * T.nStatic + s]};
        const float vy[4] = {T.vy[s], T.vy[T.nStatic + s], T.vy[2 * T.nStatic + s], T.vy[3 * T.nStatic + s]};
        c = r_poly(vx, vy, 4, X, Y, RC_OBST_FILL, RC_OBST_LINE, c);
    }
    // the creature's bodies in slot order
    for (int k = 0; k < nList; ++k) {
        const RBody &b = bodies[list[k]];
        if (b.shape == SHAPE_CIRCLE) {
            const float dx = r_sub(X, b.ax[0]), dy = r_sub(Y, b.ay[0]);
            const float d2 = r_add(r_mul(dx, dx), r_mul(dy, dy));
            if (d2 <= b.dx[0]) c = b.fill;
            if (d2 > b.dy[0] && d2 <= b.len2[0]) c = b.line;
        } else {
            bool inside = true, edge = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float cr, dt;
                r_edge(b.ax[e], b.ay[e], b.dx[e], b.dy[e], X, Y, cr, dt);
                inside = inside && cr >= 0.0f;
                edge = edge || r_band(cr, dt, b.len2[e], b.hh[e]);
            }
            c = edge ? b.line : (inside ? b.fill : c);
        }
    }
    // wall of death: 1 px wide
    {
        const float d = r_sub(X, wod);
        if (r_sq(d, d) <= r_sq(R_HALF_PX, R_HALF_PX) && Y >= R_WOD_Y0 && Y <= R_WOD_Y1) c = RC_WOD;
    }
    // flag: pole, then the triangle
    if (r_segment(R_FLAG_X, R_FLAG_Y1, R_FLAG_X, R_FLAG_Y2, X, Y)) c = RC_FLAG_LINE;
    {
        const float vx[3] = {R_FLAG_X, R_FLAG_X, R_FLAG_X2}, vy[3] = {R_FLAG_Y2, R_FLAG_Y3, R_FLAG_Y4};
        c = r_poly(vx, vy, 3, X, Y, RC_FLAG_FILL, RC_FLAG_LINE, c);
    }
    return c;
}

// grid: one workgroup per (image, tile), images outermost; block R_THREADS
__global__ __launch_bounds__(R_THREADS) void rem2d_render_kernel(State S, Terrain T, int lanes, int nEnvs, const int32_t *creatures,
                                                                  const float *cam, const uint8_t *fillRgb, const uint8_t *lineRgb,
                                                                  int W, int H, int tilesX, int tilesPerImage, uint8_t *out) {
    __shared__ RBody bodies[64];
    __shared__ int list[64];
    __shared__ int nList;
    __shared__ int obst[R_MAX_TILE_OBST];
    __shared__ int nObst;
    const int img = blockIdx.x / tilesPerImage, tile = blockIdx.x - img * tilesPerImage;
    const int tx0 = (tile % tilesX) * R_TILE_W, ty0 = (tile / tilesX) * R_TILE_H;
    const int env = creatures[img];
    if (env < 0 || env >= nEnvs) return; // (the host has refused such an index; never read outside the arena)
    const float camX = cam[2 * img], camY = cam[2 * img + 1];
    const float top = r_add(camY, r_mul((float)H, R_INV_SCALE));
    // the tile's pixel centres span [tileLX, tileUX] x [tileLY, tileUY]
    const int txl = min(tx0 + R_TILE_W, W) - 1, tyl = min(ty0 + R_TILE_H, H) - 1;
    const float tileLX = r_add(camX, r_mul((float)tx0 + 0.5f, R_INV_SCALE));
    const float tileUX = r_add(camX, r_mul((float)txl + 0.5f, R_INV_SCALE));
    const float tileUY = r_sub(top, r_mul((float)ty0 + 0.5f, R_INV_SCALE));
    const float tileLY = r_sub(top, r_mul((float)tyl + 0.5f, R_INV_SCALE));
    const float M = 2.0f * R_INV_SCALE; // cull margin: the 1-px line half width and then some
    const int t = threadIdx.x;
    if (t < 64) {
        bool keep = false;
        if (t < lanes) {
            const unsigned gl = (unsigned)(env * lanes + t);
            RBody &b = bodies[t];
            const int shape = LI(L_SHAPE);
            b.shape = shape;
            const size_t ci = (size_t)gl * 3;
            b.fill = fillRgb ? ((unsigned)fillRgb[ci] | ((unsigned)fillRgb[ci + 1] << 8) | ((unsigned)fillRgb[ci + 2] << 16))
                             : (shape == SHAPE_CIRCLE ? RC_CIRCLE_FILL : RC_BOX_FILL);
            b.line = lineRgb ? ((unsigned)lineRgb[ci] | ((unsigned)lineRgb[ci + 1] << 8) | ((unsigned)lineRgb[ci + 2] << 16))
                             : (shape == SHAPE_CIRCLE ? RC_CIRCLE_LINE : RC_BOX_LINE);
            const float px = LF(L_PX), py = LF(L_PY), hx = LF(L_HX), hy = LF(L_HY);
            const float H2 = r_sq(R_INV_SCALE, R_INV_SCALE);
            if (shape == SHAPE_CIRCLE) {
                const float ri = r_sub(hx, R_INV_SCALE), ro = r_add(hx, R_INV_SCALE);
                b.ax[0] = px; b.ay[0] = py;
                b.dx[0] = r_sq(hx, hx); b.dy[0] = r_sq(ri, ri); b.len2[0] = r_sq(ro, ro);
                b.lx = r_sub(px, hx); b.ux = r_add(px, hx); b.ly = r_sub(py, hx); b.uy = r_add(py, hx);
            } else if (shape == SHAPE_BOX) {
                const Rot q = rot_set(LF(L_ANG));
                const float lx[4] = {-hx, hx, hx, -hx}, ly[4] = {-hy, -hy, hy, hy};
                float vx[4], vy[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { // b2Mul(xf, v)
                    vx[k] = r_add(r_sub(r_mul(q.c, lx[k]), r_mul(q.s, ly[k])), px);
                    vy[k] = r_add(r_add(r_mul(q.s, lx[k]), r_mul(q.c, ly[k])), py);
                }
                b.lx = b.ux = vx[0]; b.ly = b.uy = vy[0];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int k1 = (k + 1) & 3;
                    b.ax[k] = vx[k]; b.ay[k] = vy[k];
                    b.dx[k] = r_sub(vx[k1], vx[k]); b.dy[k] = r_sub(vy[k1], vy[k]);
                    b.len2[k] = r_add(r_mul(b.dx[k], b.dx[k]), r_mul(b.dy[k], b.dy[k]));
                    b.hh[k] = r_sq(H2, b.len2[k]);
                    b.lx = fminf(b.lx, vx[k]); b.ux = fmaxf(b.ux, vx[k]); b.ly = fminf(b.ly, vy[k]); b.uy = fmaxf(b.uy, vy[k]);
                }
            }
            keep = (shape == SHAPE_BOX || shape == SHAPE_CIRCLE) && b.ux + M >= tileLX && b.lx - M <= tileUX &&
                   b.uy + M >= tileLY && b.ly - M <= tileUY;
        }
        // the bodies this tile can see, in slot order
        const unsigned long long mask = __ballot(keep);
        if (keep) list[__popcll(mask & ((1ull << t) - 1ull))] = t;
        if (t == 0) nList = __popcll(mask);
        // the obstacles whose fat AABB (0.1 m beyond the quad: more than a line's half width) meets the tile, in drawing order
        int n = 0;
        for (int base = 0; base < T.nPoly; base += 64) {
            const int s = T.nPoly - 1 - (base + t);
            const bool meets = s >= 0 && T.fux[s] >= tileLX && T.flx[s] <= tileUX && T.fuy[s] >= tileLY && T.fly[s] <= tileUY;
            const unsigned long long m = __ballot(meets);
            const int at = n + __popcll(m & ((1ull << t) - 1ull));
            if (meets && at < R_MAX_TILE_OBST) obst[at] = s;
            n += __popcll(m);
        }
        if (t == 0) nObst = n <= R_MAX_TILE_OBST ? n : -1;
    }
    __syncthreads();
    const float wod = (float)(*(const double *)(S.env8 + (size_t)E_WOD * ((size_t)S.Np * 8) + (size_t)env * 8u));
    const int row = t / (R_TILE_W / R_PX_PER_LANE), i0 = tx0 + (t % (R_TILE_W / R_PX_PER_LANE)) * R_PX_PER_LANE, j = ty0 + row;
    if (j >= H || i0 >= W) return;
    const float Y = r_sub(top, r_mul((float)j + 0.5f, R_INV_SCALE));
    unsigned px[R_PX_PER_LANE];
#pragma unroll
    for (int p = 0; p < R_PX_PER_LANE; ++p) {
        const float X = r_add(camX, r_mul((float)(i0 + p) + 0.5f, R_INV_SCALE));
        px[p] = r_shade(X, Y, T, bodies, list, nList, obst, nObst, wod);
    }
    const size_t off = (((size_t)img * H + j) * W + i0) * 3;
    if (i0 + R_PX_PER_LANE <= W && ((uintptr_t)(out + off) & 3) == 0) { // the 12 bytes as three dwords (by address: `out` may be odd)
        unsigned *o = (unsigned *)(out + off);
        o[0] = px[0] | (px[1] << 24);
        o[1] = (px[1] >> 8) | (px[2] << 16);
        o[2] = (px[2] >> 16) | (px[3] << 8);
    } else { // a row's last pixels, or rows that do not start on a dword (width not a multiple of 4)
        for (int p = 0; p < R_PX_PER_LANE && i0 + p < W; ++p) {
            out[off + 3 * p] = (uint8_t)px[p];
            out[off + 3 * p + 1] = (uint8_t)(px[p] >> 8);
            out[off + 3 * p + 2] = (uint8_t)(px[p] >> 16);
        }
    }
}

#endif
