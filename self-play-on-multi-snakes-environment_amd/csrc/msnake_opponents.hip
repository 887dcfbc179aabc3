// msnake_opponents.hip -- the scripted opponents, the board analyses and the two per-snake observations that walk every
// snake through EnvReader::snake() (windows, rays), off the step path, one translation unit.
//
// The first six files share helpers in the order they are included: wave_reduce (scripted), Board / read_board,
// wave_sum, gather_row, region_sizes and the greedy_* choosers (space), neighbours (territory).  msnake_local.inc and
// msnake_rays.inc (which uses the former's board painter) take nothing from them.  They are in this unit and not in
// msnake_views.hip because of the compiler: its interprocedural constant propagation works on EnvReader::snake() before
// the helper is inlined, what it finds depends on every caller in the unit, and only next to the callers in this unit do
// msnake_local_kernel and msnake_rays_kernel come out instruction for instruction as they were in the one-unit build
// (in msnake_views.hip they were 24 scalar instructions longer and measurably slower).
// The wave helpers, launch_by_flags and EnvReader come from msnake_device.h; the launch_* prototypes that
// msnake_capi.hip calls are in msnake_internal.h.  Nothing here is referenced by the step kernel (msnake_kernels.hip) or
// by msnake_views.hip.
#include "msnake_device.h"

#include "msnake_scripted.inc"   // msnake_scripted_actions: scripted opponents and safe-move masks
#include "msnake_space.inc"      // msnake_space_actions: reachable-space counts and the flood-fill opponent
#include "msnake_territory.inc"  // msnake_territory_actions: Voronoi territory counts and territory_greedy
#include "msnake_path.inc"       // msnake_path_actions: BFS distances to the fruits, the field and path_greedy
#include "msnake_heads.inc"      // msnake_head_fields: head distances, the Voronoi owner map and the owned counts
#include "msnake_timed.inc"      // msnake_timed_actions: cell lifetimes, the timed reach and timed_greedy
#include "msnake_local.inc"      // msnake_render_local: head-centred cell-code windows per snake
#include "msnake_rays.inc"       // msnake_render_rays: eight-direction ray observations per snake
#include "msnake_fates.inc"      // msnake_fate_actions: the fate of every move, the masks and wary_greedy
#include "msnake_explore.inc"    // msnake_explore_actions: epsilon-random moves from a stream of their own, and the draw itself
#include "msnake_playout.inc"    // msnake_playout: scripted playouts of every env in one launch, the env held in LDS
