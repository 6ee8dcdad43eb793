#!/usr/bin/env python
"""Summarise one scripts/gpu_round.sh visit (gpurun_out/<tag>/) into profiles/<tag>_*: the rocprofv3 kernel-stats
table, the bench line, the GPU test tail, and a per-kernel PMC summary (average per launch):
HBM bytes = FETCH_SIZE / WRITE_SIZE (rocprofv3 reports KB; on gfx950 FETCH_SIZE counts 128-B requests of wide
coalesced streaming reads at 64 B, so it is doubled as MI355X_MICROARCH.md "HBM" prescribes; WRITE_SIZE is
reported raw = uncalibrated), MFMA-busy and wave-cycle counters (summed over the chip)."""
import collections
import csv
import glob
import json
import os
import shutil
import sys

tag = sys.argv[1]
print_only = '--print-only' in sys.argv
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.path.join(root, 'gpurun_out', tag)
dst = os.path.join(root, 'profiles')


def short(name):
    for a in ('void ', 'ddp::(anonymous namespace)::', 'ddp::'):
        name = name.replace(a, '')
    return name.split('(')[0][:70]


def pmc(dirname):
    files = glob.glob(os.path.join(src, dirname, '**', '*counter_collection.csv'), recursive=True)
    agg = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in files:
        for r in csv.DictReader(open(f)):
            agg[short(r['Kernel_Name'])][r['Counter_Name']].append(float(r['Counter_Value']))
    return {k: {c: (sum(v) / len(v), len(v)) for c, v in d.items()} for k, d in agg.items()}


# ---- calibration of the two counters against kernels that move exactly 1 GiB (scripts/ubench/hbm_calib.hip, same box, same passes)
GIB = float(1 << 30)
calib = {}
cal_wr, cal_rd = pmc('pmc_calib_wr'), pmc('pmc_calib_rd')
for k, d in cal_wr.items():
    if 'WRITE_SIZE' in d and d['WRITE_SIZE'][0] > 0 and (k.startswith('k_store') or k.startswith('k_copy')):
        calib.setdefault(k, {})['write_factor'] = round(GIB / (d['WRITE_SIZE'][0] * 1024), 4)     # known bytes / (counter KB x 1024)
        calib[k]['write_size_raw_kb'] = round(d['WRITE_SIZE'][0], 1)
for k, d in cal_rd.items():
    if 'FETCH_SIZE' in d and d['FETCH_SIZE'][0] > 0 and (k.startswith('k_load') or k.startswith('k_copy')):
        calib.setdefault(k, {})['read_factor'] = round(GIB / (d['FETCH_SIZE'][0] * 1024), 4)
        calib[k]['fetch_size_raw_kb'] = round(d['FETCH_SIZE'][0], 1)
# the factors applied below: the non-temporal 16-B pattern is what the layer kernels' big streams use; reads keep the guide's x2
# unless the box says otherwise
WF = calib.get('k_store16_nt', {}).get('write_factor')
RF = calib.get('k_load16_nt', {}).get('read_factor') or calib.get('k_load16', {}).get('read_factor')

summary = {}
hbm = pmc('pmc_hbm_rd')
for k, d in pmc('pmc_hbm_wr').items():
    hbm.setdefault(k, {}).update(d)
for k, d in hbm.items():
    e = summary.setdefault(k, {})
    if 'FETCH_SIZE' in d:
        e['launches_profiled'] = d['FETCH_SIZE'][1]
        e['hbm_read_bytes_per_launch'] = round(d['FETCH_SIZE'][0] * 1024 * 2)      # x2: gfx950 correction
        e['fetch_size_raw_kb'] = round(d['FETCH_SIZE'][0], 1)
    if 'WRITE_SIZE' in d:
        e['hbm_write_bytes_per_launch_uncalibrated'] = round(d['WRITE_SIZE'][0] * 1024)
        if WF:
            e['hbm_write_bytes_per_launch'] = round(d['WRITE_SIZE'][0] * 1024 * WF)              # calibrated on this box
for k, d in pmc('pmc_mfma').items():
    e = summary.setdefault(k, {})
    for c in ('SQ_VALU_MFMA_BUSY_CYCLES', 'GRBM_GUI_ACTIVE', 'SQ_WAVE_CYCLES', 'SQ_WAIT_ANY'):
        if c in d:
            e[c] = round(d[c][0])
    if 'SQ_VALU_MFMA_BUSY_CYCLES' in e and e.get('GRBM_GUI_ACTIVE'):
        # GRBM_GUI_ACTIVE is summed over the 8 XCDs; MFMA busy over 1024 SIMDs
        e['mfma_busy_frac'] = round(e['SQ_VALU_MFMA_BUSY_CYCLES'] / 1024.0 / (e['GRBM_GUI_ACTIVE'] / 8.0), 4)
rows = sorted(summary.items(), key=lambda kv: -kv[1].get('GRBM_GUI_ACTIVE', 0) * kv[1].get('launches_profiled', 1))
for k, e in rows[:14]:
    print(k, json.dumps(e))
if print_only:
    sys.exit(0)
os.makedirs(dst, exist_ok=True)
out = dict(rows)
# provenance: the hash of the kernel sources the GPU box ran (scripts/gpu_round.sh wrote it next to the counters)
meta_f = os.path.join(src, 'source_sha.txt')
if os.path.exists(meta_f):
    out['_meta'] = {'source_sha': open(meta_f).read().strip().split()[0], 'tag': tag}
    if calib:
        out['_meta']['hbm_calibration'] = {
            'kernels': calib, 'write_factor_applied': WF, 'read_factor_measured': RF, 'read_factor_applied': 2.0,
            'note': 'factor = bytes the kernel moved (1 GiB) / (counter KB x 1024), scripts/ubench/hbm_calib.hip under the same rocprofv3 '
                    'passes on the same box; hbm_write_bytes_per_launch = WRITE_SIZE x write_factor_applied (k_store16_nt: full 128-B lines, '
                    "the layer kernels' q' / fragment streams); reads keep the guide's x2 (read_factor_measured beside it).  k_store_row32 "
                    '(32 B per 1-KiB row per instruction: the padded value map) is COUNTED at ~2.1x its bytes (factor 0.48): a partial-line '
                    'write costs a whole 64-B burst - that share of a kernel\'s WRITE_SIZE is real DRAM traffic above its algorithmic bytes'}
    cj = os.path.join(src, 'hbm_calib.jsonl')
    if os.path.exists(cj):
        out['_meta']['hbm_stream_rates'] = [json.loads(l) for l in open(cj) if l.startswith('{')]
rows = list(out.items())
json.dump(dict(rows), open(os.path.join(dst, f'{tag}_pmc_summary.json'), 'w'), indent=1)
for pat, name in (('prof/**/*kernel_stats.csv', f'{tag}_kernel_stats.csv'),
                  ('prof_next/**/*kernel_stats.csv', f'{tag}_kernel_stats_next_rows.csv'), ('bench.json', f'{tag}_bench.json'),
                  ('pytest_gpu.txt', f'{tag}_pytest_gpu.txt'), ('power_calibration.json', f'{tag}_power_calibration.json')):
    f = glob.glob(os.path.join(src, pat), recursive=True)
    if f:
        shutil.copy(f[0], os.path.join(dst, name))
for wl in ('ade_swin_t_k3_1x512x1024', 'city_swin_l_k10_4x1024x2048', 'kitti_depth_k20_16x352x1216', 'bev_fusion_k3_8x200x200'):
    f = glob.glob(os.path.join(src, 'prof_' + wl, '**', '*kernel_stats.csv'), recursive=True)
    if f:
        shutil.copy(f[0], os.path.join(dst, f'{tag}_{wl}_kernel_stats.csv'))
    f = os.path.join(src, f'bench_{wl}.json')
    if os.path.exists(f) and os.path.getsize(f):
        shutil.copy(f, os.path.join(dst, f'{tag}_{wl}_bench.json'))
    d = pmc('pmc_mfma_' + wl)
    if d:
        out2 = {}
        for k, e in d.items():
            r = {c: round(v[0]) for c, v in e.items()}
            if r.get('GRBM_GUI_ACTIVE'):
                r['mfma_busy_frac'] = round(r.get('SQ_VALU_MFMA_BUSY_CYCLES', 0) / 1024.0 / (r['GRBM_GUI_ACTIVE'] / 8.0), 4)
            out2[k] = r
        json.dump(out2, open(os.path.join(dst, f'{tag}_{wl}_pmc_mfma.json'), 'w'), indent=1)
for wl in ('ade_swin_t_k3_8x512x1024', 'city_swin_l_k10_4x1024x2048', 'bev_fusion_k3_8x200x200'):
    f = os.path.join(src, f'{wl}_scaling_strong_n1.json')
    if os.path.exists(f) and os.path.getsize(f):
        shutil.copy(f, os.path.join(dst, f'{tag}_{wl}_scaling_strong_n1.json'))
f = glob.glob(os.path.join(src, 'prof_fcn', '**', '*kernel_stats.csv'), recursive=True)
if f:
    shutil.copy(f[0], os.path.join(dst, f'{tag}_fcn_sampler_6_calls_kernel_stats.csv'))
f = glob.glob(os.path.join(src, 'prof_fcn_gn', '**', '*kernel_stats.csv'), recursive=True)
if f:
    shutil.copy(f[0], os.path.join(dst, f'{tag}_fcn_gn_head_kernel_stats.csv'))
for name in ('power_components.json', 'fcn_calls.log', 'fcn_gn_times.jsonl', 'call_times_bev.jsonl', 'call_times_kitti.jsonl', 'gather_by_position_init.json',
             'gather_by_position_trained.json', 'hbm_calib.jsonl', 'bench_bev_fusion_k3_r4_2x200x200.json'):
    f = os.path.join(src, name)
    if os.path.exists(f) and os.path.getsize(f):
        shutil.copy(f, os.path.join(dst, f'{tag}_{name}'))
for name in ('force_dist_rccl_world1.json', 'force_dist_rccl_world1.err'):
    f = os.path.join(src, name)
    if os.path.exists(f):
        shutil.copy(f, os.path.join(dst, f'{tag}_{name}'))
print('wrote profiles/%s_*' % tag)
