// What include/eds_hip_map.h keeps beside a handle of another header (an eds_win, an eds_imm, an eds_trk): the first eds_map_* call on
// the handle allocates it, the handle's destroy releases it.  Defined in eds_map.hip.  Nothing here is part of the ABI.
#pragma once

struct eds_map_state;

namespace edsmap_internal {
// deletes the struct (its pinned block and its device memory belong to the handle's owner, whose close() frees them); s is NULL
// afterwards.  Harmless on NULL.
void release(eds_map_state*& s);
}  // namespace edsmap_internal
