"""Per-phase instruction census of one kernel from the compiler's assembly.

    python tools/isa_census.py [--kernel interp_pool_f16x3_kernel] [--src ppsurf_amd/csrc/pps_decode.hip] [-D...] [--md out.md]
    python tools/isa_census.py --kernel f16x3 [--src ...] --md out.md       the three chip-filling split-precision kernels, one table per region

Compiles the source for gfx950 with line tables (-gline-tables-only: same code, plus `.loc` directives), takes the kernel's main loop (the
largest innermost region between a loop-header label and its back edge) and attributes every instruction to a PHASE by the source line of the
innermost inlined function it came from (PHASES below: line ranges of pps_decode.hip / pps_common.h, looked up by marker text so that edits do not
shift them), then counts by class: MFMA, other VALU (split further: conversions / packed / max3 / mov / arithmetic), LDS, vector memory, scalar,
waitcnt.  The counts are STATIC instructions of one trip of the loop = one tile of a wave (16 neighbour rows of one query).

Regions (REGIONS below) of the other two kernels, whose control flow is more than one loop:
  pointnet_fc3_feat_rows_kernel     `rows`: the row loop of feat_rows_query<true> (the smallest loop with MFMAs, first of its two copies);
                                    `producer`: the persistent loop without the two row loops (fc3 slices, exchange, per-query prologue / epilogue)
  pointnet_stn_rows_kernel<true>    `tiles3`: the query loop around stn_query_tiles<3>, first copy -- the smallest loop around the s_setprio 1 of
                                    stn_chain_h_tiles that has the most MFMAs behind it (3 x 288; with the xyz layer 3 x 292 per trip)
The last column of every table is the number of packed fp32 arithmetic ops (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32) of the phase."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '--cuda-device-only', '-S', '-gline-tables-only']


def classify(op):
    if op.startswith('v_mfma') or op.startswith('v_smfmac'):
        return 'mfma'
    if op.startswith('v_'):
        return 'valu'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'vmem'
    if op.startswith('s_waitcnt'):
        return 'wait'
    if op.startswith('s_'):
        return 'salu'
    return 'other'


def valu_kind(op):
    if op.startswith('v_cvt'):
        return 'cvt'
    if op.startswith('v_pk_'):
        return 'packed'
    if op.startswith(('v_max3', 'v_max_', 'v_min', 'v_maximum', 'v_minimum')):
        return 'max'
    if op.startswith(('v_mov', 'v_accvgpr', 'v_perm', 'v_swap', 'v_readlane', 'v_readfirstlane', 'v_writelane', 'v_permlane')):
        return 'move'
    if op.startswith(('v_exp', 'v_log', 'v_rcp', 'v_rsq', 'v_sqrt')):
        return 'transcendental'
    if op.startswith(('v_cndmask', 'v_cmp')):
        return 'select'
    if '_dpp' in op or 'dpp' in op:
        return 'dpp'
    return 'arith'


def is_packed_f32(op):
    return op.startswith(('v_pk_add_f32', 'v_pk_mul_f32', 'v_pk_fma_f32'))


def find_line(path, marker, nth=0):
    with open(path) as f:
        hits = [i + 1 for i, l in enumerate(f) if marker in l]
    if len(hits) <= nth:
        raise SystemExit('marker {!r} not found in {}'.format(marker, path))
    return hits[nth]


def phases_interp_f16x3(decode, common):
    """[(file, first line, last line, phase name)] for interp_pool_f16x3_kernel."""
    k0 = find_line(decode, 'void interp_pool_f16x3_kernel(')
    def d(marker, nth=0):
        with open(decode) as f:
            hits = [i + 1 for i, l in enumerate(f) if marker in l and i + 1 >= k0]
        return hits[nth]
    gather0 = d('const int64_t qi = ')
    split0 = d('x[kb] = split_f16_r(amax, a[2 * kb], a[2 * kb + 1]);')
    prio = d('// One streamed layer step: IH_OB output blocks')
    soft0 = d('// ---- softmax over the 64 neighbours')
    comb0 = d('float mw[4], sw[4];')
    attw0 = d('float an = 0.f;')
    join0 = d('// h3 back to fp32 (hi + lo)')
    pool0 = d('rows16_sum_transposed(a, lane);')
    end = d('range_commit(amax, range);')
    return phases_common(common)[:-1] + [
        (common, find_line(common, 'template <int KB, int NOB, int ACT, bool FENCE = true, bool INIT = false, class Sink, class Hook>'),
         find_line(common, 'sink(ob >> 1, o0, o1);'), 'dense layer loop (MFMA, fragment reads, bias)')] + phases_common(common)[-1:] + [
        (decode, gather0, split0 - 1, 'gather G rows + offset, ReLU'),
        (decode, split0, prio - 1, 'split of h1 (call site)'),
        (decode, prio, soft0 - 1, 'layer chain call sites (stream steps, sinks)'),
        (decode, soft0, comb0 - 1, 'softmax: row max / exp / row sum (DPP), stats to LDS'),
        (decode, comb0, attw0 - 1, 'softmax: combine the 4 waves, factor'),
        (decode, attw0, join0 - 1, 'attention weight of a row (mean over heads)'),
        (decode, join0, pool0 - 1, 'join call site + scale by the weight'),
        (decode, pool0, end - 1, 'pooling: transposed 16-row sums, LDS, store'),
    ]


def phases_common(common):
    """the helpers of pps_common.h every split-precision kernel is made of; the last entry is the xyz layer, the one before the weight stream"""
    c = lambda m, nth=0: find_line(common, m, nth)
    join = 'f32x4 o0 = m0 + c0, o1 = m1 + c1;'
    join_t = 'f32x4 o0 = m0[t] + c0[t], o1 = m1[t] + c1[t];'
    relu = 'for (int r = 0; r < 4; ++r) { o0[r] = fmaxf(o0[r], 0.f); o1[r] = fmaxf(o1[r], 0.f); }'
    return [
        (common, c('__device__ __forceinline__ HiLo split_f16('), c('// Range guard of the split') - 1, 'split (cvt_pkrtz hi, sub, cvt lo)'),
        (common, c('__device__ __forceinline__ void range_track('), c('__device__ __forceinline__ HiLo split_f16_r(') - 1, 'range guard (max3)'),
        (common, c('__device__ __forceinline__ void join_f16('), c('// out blocks OB0 .. OB0+NOB-1') - 1, 'join (hi + lo -> fp32)'),
        (common, c(join), c(join), 'accumulator join (main + correction)'),
        (common, c(join_t), c(join_t), 'accumulator join (main + correction)'),
        (common, c(relu, 0), c(relu, 0), 'ReLU of the layer output'),
        (common, c(relu, 1), c(relu, 1), 'ReLU of the layer output'),
        (common, c('// ---- cooperative weight-chunk streaming'), c('// XCD-aware persistent tile order') - 1, 'weight stream (global_load_lds, waits)'),
        (common, c('__device__ __forceinline__ void xyz_blocks('), c('// ---- cooperative weight-chunk streaming') - 1, 'xyz layer (K = 3 MFMA)'),
    ]


def phases_pointnet(decode, common):
    """[(file, first line, last line, phase name)] for the two PointNet kernels: the shared helpers, then the line ranges of their own functions"""
    d = lambda m, nth=0: find_line(decode, m, nth)
    c = lambda m, nth=0: find_line(common, m, nth)
    q0 = d('__device__ __forceinline__ void feat_rows_query(')
    mx0, mx_join, mx1 = d('// x <- M x: three f16 products per'), d('                o += c;'), d('a[0] = split_f16_r(amax, x0[0], x0[1]);', 1)
    logit = d('for (int r = 0; r < 4; ++r) s += w0[r] * o0[r] + w1[r] * o1[r];')
    soft0, soft_upd, q1 = d('// online softmax: advance the state'), d('acc[bb][r] = acc[bb][r] * scale + en * y[bb][r];'), d('const float inv = 1.f / row16_sum(ssum);')
    t0, t1 = d('__device__ __forceinline__ void stn_chain_h_tiles('), d('__device__ __forceinline__ void stn_query_tiles(')
    t2 = d('// H = false: fp32 (wdense = wpack + 256 floats of the same image)')
    k0 = d('void pointnet_fc3_feat_rows_kernel(')
    return phases_common(common) + [
        (common, c('template <int KB, int NOB, int ACT, bool FENCE = true, bool INIT = false, class Sink, class Hook>'), c('sink(ob >> 1, o0, o1);'),
         'dense layer loop (MFMA, fragment reads, bias)'),
        (common, c('template <int T, int KB, int NOB, int ACT, bool FENCE = true, class Sink>'), c('sink(t, ob >> 1, o0, o1);'),
         'dense layer loop, T tiles (MFMA, fragment reads, bias)'),
        (common, c('__device__ __forceinline__ float row16_max('), c('// max(a, b) as ONE v_max_f32') - 1, 'row reductions (DPP)'),
        (common, c('// max(a, b) as ONE v_max_f32'), c('// ---- value of lane (l ^ st)') - 1, 'maxima (max_raw, max3_raw, row16_max4)'),
        (common, c('// Sum over the 16 rows of EVERY channel'), c('// ---- dense layer on a register tile') - 1, 'pooling: transposed 16-row sums'),
        (decode, mx_join, mx_join, 'M x: accumulator join'),
        (decode, mx0, mx1 - 1, 'M x: MFMAs from registers, ReLU'),
        (decode, logit, logit, 'attention logit (w . y)'),
        (decode, soft_upd, soft_upd, 'online softmax: acc * scale + en * y'),
        (decode, soft0, q1 - 1, 'online softmax: state (max, exp, sum)'),
        (decode, q0, q1 + 3, 'feat_rows_query: the rest (coordinates, call sites, store)'),
        (decode, t0, t1 - 1, 'stn_chain_h_tiles (call sites, sinks, stream steps)'),
        (decode, t1, t2 - 1, 'stn_query_tiles (coordinates, tile maximum, store)'),
        (decode, k0, d('range_commit(amax, flag);', 2), 'fc3 producer + kernel body (exchange buffers, barriers)'),
    ]


def backward_spans(body):
    """(first line, last line) of every region between a label and the LAST branch back to it"""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r'(\.LBB\d+_\d+):', l)] if m}
    spans = {}
    for i, l in enumerate(body):
        m = re.match(r'\s*s_cbranch_\w+\s+(\.LBB\d+_\d+)', l) or re.match(r'\s*s_branch\s+(\.LBB\d+_\d+)', l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            spans[labels[m.group(1)]] = i
    return sorted(spans.items())


def count_mfma(body, a, b):
    return sum(1 for l in body[a:b + 1] if re.match(r'\s+v_s?mfmac?', l))


def regions_of(kernel, body, files, decode):
    """[(region name, [(first, last), ...] line ranges of `body`, what one pass over the region is)]"""
    spans = backward_spans(body)
    main_loop = max(spans, key=lambda ab: ab[1] - ab[0])
    if 'fc3_feat_rows' in kernel:
        inner = [ab for ab in spans if main_loop[0] < ab[0] and ab[1] < main_loop[1] and count_mfma(body, *ab) > 0]
        small = min(inner, key=lambda ab: ab[1] - ab[0])
        n = count_mfma(body, *small)
        copies, cur = [], None                    # the row loop has two copies (first / second query of a wave); labels of one copy overlap
        for ab in sorted(x for x in inner if count_mfma(body, *x) == n):
            if cur is not None and ab[0] <= cur[1]:
                cur = (cur[0], max(cur[1], ab[1]))
            else:
                if cur is not None:
                    copies.append(cur)
                cur = ab
        copies.append(cur)
        rest, at = [], main_loop[0]
        for a, b in copies:
            rest.append((at, a - 1))
            at = b + 1
        rest.append((at, main_loop[1]))
        return [('producer', rest, 'one pass = 16 queries of a workgroup: the persistent loop WITHOUT the row loops of feat_rows_query<true>'),
                ('rows', [copies[0]], 'one trip = one 16-row tile of a query: the row loop of feat_rows_query<true>, first of {} copies'.format(len(copies)))]
    if 'stn_rows' in kernel:
        # stn_chain_h_tiles<T> raises the priority in front of its dense layers (288 T MFMAs): the stretch behind an s_setprio 1 with the most MFMAs
        # up to the next s_setprio belongs to T = 3, and the smallest loop around its head is the query loop of the three-tile passes
        prio = [i for i, l in enumerate(body) if re.match(r'\s+s_setprio\s', l)] + [len(body) - 1]
        heads = [(count_mfma(body, a, b), -a) for a, b in zip(prio, prio[1:]) if re.match(r'\s+s_setprio\s+1', body[a])]
        head = -max(heads)[1]
        a, b = min((ab for ab in spans if ab[0] <= head <= ab[1]), key=lambda ab: ab[1] - ab[0])
        return [('tiles3', [(a, b)], 'one trip = three 16-row tiles of one query: the loop around stn_query_tiles<3>, first copy')]
    return [('loop', [main_loop], 'one trip = one 16-row tile of a wave')]


def census(kernel, body, files, ranges, phases):
    table = collections.OrderedDict((p[3], collections.Counter()) for p in phases)
    table['(other lines)'] = collections.Counter()
    vk = collections.OrderedDict((name, collections.Counter()) for name in table)
    for lo, hi in ranges:
        cur = (None, 0)
        for i in range(lo, -1, -1):                    # the .loc state at the head of the range: the last .loc before it
            m = re.match(r'\s*\.loc\s+(\d+)\s+(\d+)', body[i])
            if m:
                cur = (files.get(int(m.group(1))), int(m.group(2)))
                break
        for l in body[lo:hi + 1]:
            m = re.match(r'\s*\.loc\s+(\d+)\s+(\d+)', l)
            if m:
                cur = (files.get(int(m.group(1))), int(m.group(2)))
                continue
            m = re.match(r'\s+([a-z_0-9]+)', l)
            if not m or l.strip().startswith(('.', ';')):
                continue
            op = m.group(1)
            name = '(other lines)'
            for f, a, b, nm in phases:
                if cur[0] and os.path.basename(cur[0]) == os.path.basename(f) and a <= cur[1] <= b:
                    name = nm
                    break
            c = classify(op)
            table[name][c] += 1
            if c == 'valu':
                vk[name][valu_kind(op)] += 1
                if is_packed_f32(op):
                    vk[name]['pk_f32'] += 1
    return table, vk


def render(kernel, region, what, ranges, table, vk):
    classes = ['mfma', 'valu', 'lds', 'vmem', 'salu', 'wait', 'other']
    kinds = ['cvt', 'packed', 'max', 'move', 'arith', 'select', 'transcendental', 'dpp']
    tot, allk = collections.Counter(), collections.Counter()
    for c in table.values():
        tot.update(c)
    for c in vk.values():
        allk.update(c)
    out = ['| phase | ' + ' | '.join(classes) + ' | VALU by kind (' + ' / '.join(kinds) + ') | packed f32 (add / mul / fma) |', '|---|' + '---|' * (len(classes) + 2)]
    for name, c in table.items():
        if sum(c.values()) == 0:
            continue
        out.append('| {} | {} | {} | {} |'.format(name, ' | '.join(str(c[k]) for k in classes), ' / '.join(str(vk[name][k]) for k in kinds), vk[name]['pk_f32']))
    out.append('| **total** | {} | {} | **{}** |'.format(' | '.join('**{}**'.format(tot[k]) for k in classes), ' / '.join(str(allk[k]) for k in kinds), allk['pk_f32']))
    head = ('kernel `{}`, region `{}`: {} assembly lines ({} instructions), VALU : MFMA = {:.2f} (static; {})'
            .format(kernel, region, sum(b - a + 1 for a, b in ranges), sum(tot.values()), tot['valu'] / max(1, tot['mfma']), what))
    return head + '\n\n' + '\n'.join(out) + '\n'


F16X3_KERNELS = ['interp_pool_f16x3_kernel', 'pointnet_stn_rows_kernelILb1E', 'pointnet_fc3_feat_rows_kernel']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel', default='interp_pool_f16x3_kernel', help='a kernel name as it is mangled (a template argument as ILb1E), or f16x3 for the three big ones')
    ap.add_argument('--src', default=os.path.join(REPO, 'ppsurf_amd', 'csrc', 'pps_decode.hip'))
    ap.add_argument('--md', default=None)
    ap.add_argument('--keep', default=None, help='write the assembly here')
    args, extra = ap.parse_known_args()
    common = os.path.join(os.path.dirname(os.path.abspath(args.src)), 'pps_common.h')
    out = args.keep or os.path.join(tempfile.mkdtemp(), 'k.s')
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')] + FLAGS + extra + ['-o', out, args.src], stderr=subprocess.DEVNULL)
    lines = open(out).read().split('\n')
    files = {}
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            files[int(m.group(1))] = os.path.normpath(os.path.join(m.group(2), m.group(3)) if m.group(3) else m.group(2))
    texts = []
    for kernel in (F16X3_KERNELS if args.kernel == 'f16x3' else [args.kernel]):
        start = next(i for i, l in enumerate(lines) if re.match(r'_Z\d+' + kernel + r'\w*:', l))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
        body = lines[start:end]
        if 'interp_pool_f16x3' in kernel:
            phases = phases_interp_f16x3(args.src, common)
        elif 'pointnet' in kernel:
            phases = phases_pointnet(args.src, common)
        else:
            phases = []
        whole = sum(1 for l in body if re.match(r'\s+v_pk_(add|mul|fma)_f32', l))
        for region, ranges, what in regions_of(kernel, body, files, args.src):
            table, vk = census(kernel, body, files, ranges, phases)
            texts.append(render(kernel, region, what, ranges, table, vk))
        texts.append('whole function `{}` (every path): {} MFMA, {} packed f32 ops\n'.format(kernel, count_mfma(body, 0, len(body) - 1), whole))
    text = '\n'.join(texts)
    print(text)
    if args.md:
        with open(args.md, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
