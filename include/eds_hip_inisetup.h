/* eds_hip_inisetup.h — the rest of dso::CoarseInitializer::setFirst on the device (reference src/init/CoarseInitializer.cpp:688-773,
 * lines quoted as :n; src/init/CoarseInitializer.h:81-297, quoted as H:n): the pixel status of the upper levels (makePixelStatus with
 * gridMaxSelection) and makeNN.  With these, a caller gives eds_ini_set_first the first frame and eds_ini_setup_levels a selector
 * that holds the same image, and the handle is ready for eds_ini_track_frame: no status map and no table crosses the bus on the
 * caller's behalf.  The symbols are exported by libeds_hip.so; the object is eds_hip_init.h's eds_ini, and no entry point of that
 * header changes.
 *
 * Conventions are those of eds_hip_init.h: EDS_OK or a negative eds_status, eds_last_error() for the text.  EDS_ERR_INVALID for a NULL
 * handle or required argument, a level out of range, a density or threshold factor that is not positive and finite, recursions_left
 * outside 0 .. 64, a selector of another size or device, a level below one with no points (the rule of eds_ini_make_nn), more selected
 * pixels than max_points_per_level.  EDS_ERR_STATE before what a call reads exists: eds_ini_make_pixel_status before eds_ini_set_first,
 * eds_ini_set_points_status and eds_ini_get_pixel_status before the level's map (a new eds_ini_set_first forgets the maps),
 * eds_ini_make_neighbours before the points of the level and of the level above, eds_ini_get_neighbours before
 * eds_ini_make_neighbours (or after the points or the tables were replaced), eds_ini_setup_levels before the first frame or the
 * selector's image.  Every check is made before the device is touched, and nothing changes on an error — except the count of selected
 * pixels against max_points_per_level, which is known only after the compaction (as for eds_ini_set_points: the level is then without
 * points).
 *
 * What is restated.
 *  1. gridMaxSelection (H:84-240).  The pot x pot cells start at (1, 1) and step by pot while x < w - pot, y < h - pot.  Per pixel
 *     sqgd = dx dx + dy dy in fp32 without contraction, TH = (THFac 10) 0.75, the test sqgd > TH TH, the scores |dx|, |dy|, |dx - dy|,
 *     |dx + dy|.  Each of a cell's four winners is the FIRST pixel in the visiting order (dx outer, dy inner) that has the cell's
 *     largest score, and a score of 0 never wins: the strict > of H:114-123 against a best that starts at 0.  pot is a run-time value
 *     (the templates 1 .. 11 and the generic form compute the same); a level with h - pot <= 1 or w - pot <= 1 has no cells and 0
 *     points.  On the device a lane (pot <= 8) or a wavefront (pot > 8) owns a cell; the wavefront folds its lanes' candidates by
 *     (larger score, then smaller visiting rank), which gives the serial loop's winner.  numGood is the number of set pixels.
 *  2. makePixelStatus's controller (H:243-297) is host code inside the library: quotia, newSparsity = (int)(sparsity sqrtf(quotia) +
 *     0.7f), the THFac = 0.5 switch, the three-way stop test.  sqrtf is taken on the host.  One 4-byte count comes back per pass, and
 *     there are at most recursions_left + 1 passes.  The reference's global sparsityFactor (settings.cpp:212, initial value 5) is
 *     state of the handle.  Where the reference's float-to-int conversion would overflow, the new sparsity is 2^30.
 *  3. makeNN (:884-958) with the reference's tables, ties included — eds_ini_make_nn's (eds_hip_init.h item 4): the k-d tree
 *     nanoflann builds over the level (leaf size 5) and over the level above, walked as nanoflann walks it, the ten neighbours in
 *     nanoflann's order; the parent is nanoflann's one nearest point of the level above to 0.5f u - 0.25f; fewer than 10 points
 *     leave -1.  The build is host code (csrc/eds_nntree.hpp): eds_ini_make_neighbours READS BACK THE PACKED (u, v) of the level and
 *     of the level above (8 n + 8 n_up bytes), builds the two trees, and uploads their nodes and index arrays (at most 52 bytes a
 *     point).  The walk is the same header's on the device, a query per lane, its stack of pending far sides (one per level of the
 *     tree, at most 64) in the lane's private memory; distances are d0 d0 + d1 d1 of the fp32 u, v without contraction.  A level
 *     whose tree is deeper than 64 — points on the pixel lattice never give one — is walked on the host and its table uploaded.
 *  4. What eds_ini_set_neighbours derives from the tables — the dependency schedule and the child lists — stays host code
 *     (csrc/eds_init.hpp, unchanged).  For it eds_ini_make_neighbours READS THE TABLES BACK ONCE per level (n x 11 int32) and uploads
 *     the schedule as eds_ini_set_neighbours does.  With item 3's (u, v) these are the set-up's read-backs besides the counts.
 *
 * The host restatement (csrc/eds_inisetup.hpp: edsini::grid_max_selection, edsini::make_pixel_status in the reference's loop order;
 * edsini::make_nn of csrc/eds_init.hpp over csrc/eds_nntree.hpp) and the device agree bit for bit on everything this header returns.
 *
 * Out of scope.  Building the tree on the device.  FullSystem::initializeFromInitializer, which is not in the reference tree.  An LDS-resident optReg.  Deriving the schedule on the
 * device.
 */
#ifndef EDS_HIP_INISETUP_H_
#define EDS_HIP_INISETUP_H_

#include "eds_hip_init.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EDS_HIP_INISETUP_ABI_VERSION 1
int eds_ini_setup_abi_version(void);

#define EDS_INI_SPARSITY_START 5
#define EDS_INI_NN_TILE 256                    /* queries per workgroup of the neighbour search */

/* the reference's global `sparsityFactor`: it starts at 5, every eds_ini_make_pixel_status reads it and leaves what the reference
 * leaves, across levels and across a second eds_ini_set_first.  Neither call touches the device. */
int eds_ini_get_sparsity(const eds_ini* ini, int32_t* out);
int eds_ini_set_sparsity(eds_ini* ini, int32_t value);        /* value < 1 is taken as 1, as H:245 does; above 2^30 as 2^30 */

/* makePixelStatus(firstFrame->dIp[lvl], map, w[lvl], h[lvl], desired_density, recursions_left, th_factor) on the pyramid
 * eds_ini_set_first left in device memory; lvl 0 .. levels - 1 (the reference only uses it for lvl >= 1).  The map stays on the
 * device.  n_good_out: the returned numGoodPoints; passes_out: how many gridMaxSelection passes ran (1 .. recursions_left + 1).
 * Either may be NULL. */
int eds_ini_make_pixel_status(eds_ini* ini, int lvl, float desired_density, int recursions_left, float th_factor, int32_t* n_good_out,
                              int32_t* passes_out);
/* the level's map, h x w bytes, 0 / 1: for tests */
int eds_ini_get_pixel_status(eds_ini* ini, int lvl, uint8_t* map_out);
/* the level's points from that map (my_type 1, :733), with no upload: what eds_ini_set_points leaves for the same map as floats.
 * n_out may be NULL. */
int eds_ini_set_points_status(eds_ini* ini, int lvl, int32_t* n_out);

/* makeNN for one level from the points on the device: the tables eds_ini_make_nn would fill for the same points (nanoflann's), then everything
 * eds_ini_set_neighbours does with them.  The level above must have points (and at least one) unless lvl is the top level. */
int eds_ini_make_neighbours(eds_ini* ini, int lvl);
/* those tables: neighbours n x 10, parent n (NULL at the top level) */
int eds_ini_get_neighbours(eds_ini* ini, int lvl, int32_t* neighbours, int32_t* parent);
/* the device time of the last eds_ini_make_neighbours' search kernel in milliseconds (two events around its launch; 0 for a level
 * without points) */
int eds_ini_get_neighbours_kernel_ms(const eds_ini* ini, float* ms_out);

/* setFirst :694-764 after eds_ini_set_first.  The selector holds the same image (eds_sel_set_image), is on the same device and of the
 * same H x W.  Per level currentPotential = 3 (:702).  Level 0 is makeMaps(density[0], 1, th 2) + eds_ini_set_points_selected;
 * levels 1 .. are eds_ini_make_pixel_status(density[l], 5, 1) + eds_ini_set_points_status; then makeNN for every level, top first.
 * densities (one per level) NULL: {0.03f, 0.05f, 0.15f, 0.5f, 1.f}; density[l] = (densities[l] * (float)W) * (float)H in fp32, as
 * :705-707 forms it.  n_out (levels entries, may be NULL): the points per level. */
int eds_ini_setup_levels(eds_ini* ini, eds_sel* sel, const float* densities, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* EDS_HIP_INISETUP_H_ */
