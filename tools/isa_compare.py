"""Function-by-function comparison of two device builds of the kernel sources: instruction text (branch labels
normalised) and the resource usage the compiler reports.  Used to check that a change leaves existing kernels' code alone.

    for f in fjsp_kernels fjsp_group fjsp_lp_device fjsp_lp_global fjsp_env fjsp_arrivals fjsp_snapshot fjsp_rollout_buffer fjsp_ppo \\
             fjsp_mlp_train fjsp_policy_mlp fjsp_generate; do
      # (every .hip with kernels) once in a checkout of the parent (-> DIR_A), once in this tree (-> DIR_B)
      hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function -I include \\
            -I deep_reinforcement_learning_for_fjsp_amd/csrc --cuda-device-only -S \\
            deep_reinforcement_learning_for_fjsp_amd/csrc/$f.hip -o DIR/$f.s -Rpass-analysis=kernel-resource-usage 2> DIR/$f.rpass
    done
    python tools/isa_compare.py DIR_A DIR_B

Prints one line per function of DIR_A (SAME / DIFF instruction text, res= / res! resource usage, instruction counts,
VGPRs) and one per function only DIR_B has (NEW), then the count of identical functions.
"""
import glob
import os
import re
import sys


def parse_asm(path):
    out, cur, n, body = {}, None, 0, []
    for line in open(path):
        m = re.match(r'^(_Z\S+):\s*(;.*)?$', line)
        if m:
            cur, n, body = m.group(1), 0, []
            continue
        if cur and line.startswith('.Lfunc_end'):
            out[cur] = (n, body)
            cur = None
            continue
        if cur:
            s = line.strip()
            if s and not s.startswith(('.', ';')) and not s.endswith(':'):
                n += 1
                body.append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s+;.*$', '', s)))
    return out


def parse_remarks(path):
    d, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            d[cur] = {}
            continue
        m = re.search(r"remark: .*? ([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur:
            d[cur][m.group(1).strip()] = int(m.group(2))
    return d


def main(a, b):
    same = total = 0
    for f in sorted(os.path.basename(p)[:-2] for p in glob.glob(os.path.join(a, "*.s"))):
        fa, fb = parse_asm("%s/%s.s" % (a, f)), parse_asm("%s/%s.s" % (b, f))
        ra, rb = parse_remarks("%s/%s.rpass" % (a, f)), parse_remarks("%s/%s.rpass" % (b, f))
        for k in sorted(fa):
            total += 1
            st = k in fb and fa[k][1] == fb[k][1]
            sr = ra.get(k) == rb.get(k)
            same += st and sr
            print("%-4s %-4s insts %6d -> %6s  VGPRs %s  %s" % ("SAME" if st else "DIFF", "res=" if sr else "res!", fa[k][0],
                                                             fb[k][0] if k in fb else "-", ra.get(k, {}).get("VGPRs", "?"), k))
        for k in sorted(set(fb) - set(fa)):
            print("NEW            insts %6d  VGPRs %s  %s" % (fb[k][0], rb.get(k, {}).get("VGPRs", "?"), k))
    print("identical (instruction text + resource usage): %d / %d functions of the first build" % (same, total))
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
