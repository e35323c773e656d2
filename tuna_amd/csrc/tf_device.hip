// tf_device.hip -- the one translation unit behind the C ABI of libtunafock.so (include/tunafock.h): the kernel headers, then the host
// units in the order their text always stood in (which unit holds what).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <array>
#include <cstring>
#include <condition_variable>
#include <dlfcn.h>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/tunafock.h"
#include "tf_internal.h"
#include "tf_kernels.hip.h"
#include "tf_jkpacked.hip.h"
#include "tf_packed_host.h"
#include "tf_tiles_host.h"
#include "tf_jk_plan.h"
#include "tf_jktile.hip.h"
#include "tf_eri.hip.h"
#include "tf_eri_team.hip.h"
#include "tf_eri_teamc.hip.h"
#include "tf_eri_team_api.h"
#include "tf_eri_plan.h"
#include "tf_oneel.hip.h"
#include "tf_scf.hip.h"
#include "tf_mp2.hip.h"
#include "tf_mp3.hip.h"
#include "tf_ccd.hip.h"
#include "tf_ccsd.hip.h"
#include "tf_cis.hip.h"
#include "tf_ucis.hip.h"
#include "tf_cisd.hip.h"
#include "tf_mp4.hip.h"
#include "tf_mp2dens.hip.h"
#include "tf_triples.hip.h"
#include "tf_dft.hip.h"
#include "tf_xckernel.hip.h"
#include "tf_ctx_plan.h"
#include "tf_shard_plan.h"

// ---- the context and its three lifetimes; the ranks of a sharded tensor; the basis and the one-electron entry points -------------
#include "tf_ctx.hip.h"
#include "tf_ranks_host.hip.h"
#include "tf_basis_host.hip.h"

extern "C++" {
static int tile_list_upload(tf_ctx *ctx, const tft::TaskList &TL, bool own_shapes, tf_ctx::TileList &D);   // (tf_jk_host.hip.h; the tensor build uploads the first list)
}

extern "C" {

int tf_version(void) { return 100; }

// ---- the tensor build: uploads, struct EriBuild and its units, tf_build_eri, the tensor queries.  Included HERE,
// above the Fock build: the order in which the kernel templates are first used decides the order of the kernels in the code object.
#include "tf_eri_host.hip.h"

// ---- the Fock build: state of a tensor build, passes per layout, entry points.  Included HERE: the order in
// which the kernel templates are first used decides the order of the kernels in the code object, which stays what it was. -------------
#include "tf_jk_host.hip.h"
int EriBuild::alloc_jk_scratch() { return jk_alloc_state(ctx); }

static void offer_symmetry(tf_ctx *ctx, tfscf::Workspace &w, int n);   // (tf_scf_entry.hip.h; tf_natural_orbitals offers it too)

// ---- Kohn-Sham exchange-correlation (next row of the hot path: SURVEY.md section 8f rank 2) --------------------------

#include "tf_dft_host.hip.h"

// ---- AO->MO transformation, MP2 ... CCSD(T), the MP2 density: the drivers of the correlated methods (consumers of the resident tensor) ----
#include "tf_corr_host.hip.h"
// ---- CIS / TDHF, TD-DFT / TDA, the stability analysis, CIS(D): the drivers of the excited states, on the shared pieces of the above ----
#include "tf_excited_host.hip.h"

// ---- the eigensolver entry points and the five native SCF cycles ------------------------------------------------------------------
#include "tf_scf_entry.hip.h"

}  // extern "C"
