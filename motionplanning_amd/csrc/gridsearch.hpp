// gridsearch.hpp — what the grid planners' kernels share: astar.hip (node tables in LDS, up to 51 x 51 cells) and
// gridbig.hip (node tables in a global workspace, up to MP_GRID_MAX_CELLS).
#pragma once
#include "../../include/mp_jlmath.h"
#include "runtime.hpp"

enum { AS_ASTAR = 0, AS_DKA = 1, AS_BFS = 2 };  // the planner of as_launch / gb_launch (MP_GRID_*)

struct AsArgs {
  int nx, ny;
  int per_scene;  // searches per scene: 1 (start cells in scell), or nx*ny (search q starts in cell q + 1)
  int cap;        // pop cap
  const double* geo;          // [scenes][4]
  const int* scell;           // [searches][2] starting_pos (per_scene == 1)
  const int* gcell;           // [scenes][2] ending_pos
  const unsigned char* mask;  // [scenes][nx*ny]
  double* cost;               // [searches] final_cost (null: breadth-first search has none)
  int *found, *pops, *n_nodes;  // [searches] (each may be null)
  int* pop_seq;               // [searches][cap] Encode index per pop, or null
  int* path;                  // [searches][nx*ny + 1] astarpath as Encode indices, start -> goal, or null
  int* path_n;                // [searches]
  double* path_len;           // [searches] astar.r.path_length, or null
  int* err;                   // [1] a search reached the pop cap
};

// sum(norm(actualpath[i+1, :] - actualpath[i, :])) (astar_utils.jl:129, dka_utils.jl:112), a left fold over
// the path's cnt cells, held goal side first in rev
template <typename T>
__device__ __forceinline__ double as_path_length(const T* rev, int cnt, int nx, int sx, int sy, double xf, double yf,
                                                 const double* ge) {
  double acc = 0.0;
  double ax = 0.0, ay = 0.0;
  for (int i = 0; i < cnt; i++) {
    const int c = rev[cnt - 1 - i];
    const int px = c == 0 ? sx : (c - 1) % nx + 1, py = c == 0 ? sy : (c - 1) / nx + 1;
    const double tx = ((double)px - 1.0) * xf + ge[0], ty = ((double)py - 1.0) * yf + ge[1];
    if (i > 0) {
      const double ex = tx - ax, ey = ty - ay;
      const double n = mpj_sqrt(ex * ex + ey * ey);
      acc = i == 1 ? n : acc + n;
    }
    ax = tx;
    ay = ty;
  }
  return acc;
}

// gridbig.hip: bytes of node workspace (WS_GB_NODE) the global-memory kernels need for `searches` searches of
// nx*ny = N cells, and their launch on the context stream (A complete: mask, err and cap set)
size_t gb_node_bytes(int planner, size_t searches, int N);
int gb_launch(mp_ctx* ctx, int planner, int searches, void* node_ws, const AsArgs& A);

// astar.hip: defineAstar's factors (ge = [xmin, ymin, x_factor, y_factor]) and real -> cell conversion on the host
bool as_factors(const double* b, int nx, int ny, double* ge);
bool as_cell(const double* ge, const double* real, int* cell);
