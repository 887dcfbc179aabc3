// msnake_views.hip -- the kernels off the step path that export, copy or render a handle's state, one translation unit.
//
// The wave helpers, the HV_SET* record-word writers (state import), launch_by_flags and EnvReader come from
// msnake_device.h; the four files take nothing from each other.  The launch_* prototypes that msnake_capi.hip calls are in
// msnake_internal.h.  Nothing here is referenced by the step kernel (msnake_kernels.hip) or by msnake_opponents.hip.
// (msnake_local.inc and msnake_rays.inc are views too, but live in msnake_opponents.hip: see there.)
#include "msnake_device.h"

#include "msnake_state.inc"   // msnake_get_state / msnake_set_state: the canonical state words <-> the device layout
#include "msnake_generate.inc"  // msnake_generate_states: random legal positions in those words, built on the device
#include "msnake_hash.inc"   // msnake_hash_states: a 64-bit hash of every env's canonical words
#include "msnake_copy.inc"   // msnake_copy_envs: env state copied between two handles on the device
#include "msnake_causes.inc"  // msnake_death_causes: why each snake died and on whose body, from two states one step apart
#include "msnake_cells.inc"   // msnake_render_cells: the observation as cell codes and the per-snake table
#include "msnake_agents.inc"  // msnake_agent_outcomes: per-snake rewards, deaths and episode totals behind a step
