"""CPU only: which status wins.  The *_host.py files pin one bad argument at a time; this one replays every single bad argument AND every
pair of bad arguments of tests/api_calls.py against the built library and compares each entry point's statuses, whole, with the record in
tests/api_status.json -- the behaviour of the library before its argument checks were folded into shared helpers.  The record is compared and
never rewritten from the code under test: an entry changes only by hand, with the line of d3f_api.hip that changes the precedence as the reason.

The rows carry made-up device addresses.  Every recorded row is rejected on the host, and where no device exists a call that slips through a
lost check comes back as D3F_ERR_HIP, which is not in the record.  On a machine with a GPU the module does not run at all."""
import pytest
import torch

if torch.cuda.device_count() > 0:
    pytest.skip("made-up device addresses: only where nothing can be launched", allow_module_level=True)

import itertools  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402

import api_calls as AC  # noqa: E402

# every entry point whose body (or a static helper under it) states its checks through the shared helpers of d3f_api.hip
EDITED = [
    "d3f_pcd_to_index", "d3f_vox_idx_iou", "d3f_voxel_downsample", "d3f_mesh_count", "d3f_mesh_extract", "d3f_volume_gaussian", "d3f_volume_sample",
    "d3f_volume_sample_backward", "d3f_band_mark", "d3f_band_sample", "d3f_band_sample_backward", "d3f_volume_edt", "d3f_volume_components",
    "d3f_volume_components_linked", "d3f_volume_links", "d3f_volume_flow", "d3f_volume_pool", "d3f_part_motion", "d3f_volume_geodesic_init",
    "d3f_volume_geodesic_relax", "d3f_volume_geodesic_finish", "d3f_volume_follow", "d3f_volume_segments", "d3f_path_shorten", "d3f_volume_peaks",
    "d3f_volume_align_accumulate", "d3f_volume_raycast",
]


@pytest.fixture(scope="module")
def table():
    with open(AC.RECORD) as fh:
        return json.load(fh)["calls"]


def test_record_covers_every_edited_entry_point(table):
    assert sorted(table) == sorted(AC.BY_NAME) and set(EDITED) <= set(table)
    assert os.path.getsize(AC.RECORD) < os.path.getsize(os.path.join(AC.HERE, "plan_names.json"))
    for fn, rec in table.items():
        kept = AC.unranges(rec["kept"])
        assert rec["rows"] == len(AC.BY_NAME[fn].rows()), (fn, "the generator and the record list different rows")
        assert kept == sorted(set(kept)) and kept and 0 <= kept[0] and kept[-1] < rec["rows"] and len(kept) == len(rec["status"]), fn
        assert set(rec["status"]) <= set(AC.VALIDATION), (fn, "a recorded row is one the library rejects before any launch")


@pytest.mark.parametrize("fn", sorted(AC.BY_NAME))
def test_record_holds_every_status_and_every_pair_of_statuses(table, fn):
    """from the record alone: a single bad argument for every status the entry point can return, two bad arguments for every pair of them"""
    spec, rec = AC.BY_NAME[fn], table[fn]
    rows = spec.rows()
    status = dict(zip(AC.unranges(rec["kept"]), rec["status"]))
    single = {rows[i][0]: s for i, s in status.items() if len(rows[i]) == 1}
    assert set(single.values()) == spec.statuses, fn
    pairs = {frozenset((single[rows[i][0]], single[rows[i][1]])) for i in status
             if len(rows[i]) == 2 and rows[i][0] in single and rows[i][1] in single}
    missing = [p for p in itertools.combinations(sorted(spec.statuses), 2) if frozenset(p) not in pairs]
    assert not missing, (fn, missing)


@pytest.mark.parametrize("fn", sorted(AC.BY_NAME))
def test_statuses_equal_the_record(table, fn):
    lib = AC.load()
    spec, rec = AC.BY_NAME[fn], table[fn]
    kept = AC.unranges(rec["kept"])
    got = AC.replay(lib, spec, kept)
    rows = spec.rows()
    wrong = ["%s: recorded %d, now %d" % (spec.describe(rows[i]), w, g) for i, g, w in zip(kept, got, rec["status"]) if g != w]
    print("%s: %d rows, %d differ" % (fn, len(kept), len(wrong)))
    assert got == rec["status"], "%d of %d rows of %s differ from the record:\n%s" % (len(wrong), len(kept), fn, "\n".join(wrong[:40]))
