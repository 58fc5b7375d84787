"""The kernels of ppg_posterior per workload, from a rocprofv3 kernel trace of `tools/bench_posterior.py --trace-only`:

    python tools/posterior_kernel_split.py posterior_kernel_trace.csv > profiles/posterior_kernel_split.txt

--trace-only makes three calls of every workload, the six graphs at 1, then 64, then 2048 utterances.  A library call
begins with align_prepare; a batch that engine.posterior_items splits is several library calls, whose times are added
until the grids of posterior_forward<1> (which every call launches over all its items) have covered the workload's
utterances.  Printed: microseconds per kernel, the median of the three calls; both instances of a pass are one column."""
import collections
import csv
import sys

KERNELS = ['align_prepare', 'viterbi_check', 'posterior_check', 'posterior_forward', 'posterior_backward']
GRAPHS = ['model', 'chain', 'optional', 'sausage', 'loop10', 'loop170']
SHAPES = [1, 64, 2048]


def main():
    with open(sys.argv[1]) as file:
        rows = sorted(csv.DictReader(file), key=lambda row: int(row['Start_Timestamp']))
    calls = []
    for row in rows:
        name = next((kernel for kernel in KERNELS if kernel in row['Kernel_Name']), None)
        if name is None or (name != 'align_prepare' and not calls):
            continue
        if name == 'align_prepare':
            calls.append(collections.Counter())
        calls[-1][name] += int(row['End_Timestamp']) - int(row['Start_Timestamp'])
        if name == 'posterior_forward' and ('<1>' in row['Kernel_Name'] or 'ILi1E' in row['Kernel_Name']):
            calls[-1]['items'] += int(row['Grid_Size_X']) // int(row['Workgroup_Size_X'])
    calls = iter(calls)
    print('utterances graph ' + ' '.join(KERNELS) + '   (microseconds, median of three calls, 1000 frames)')
    for items in SHAPES:
        for graph in GRAPHS:
            three = []
            for _ in range(3):
                whole = collections.Counter()
                while whole['items'] < items:
                    whole.update(next(calls))
                three.append(whole)
            print(f'{items:5d} {graph:9s}' + ' '.join(f'{sorted(call[k] for call in three)[1] / 1000:10.1f}' for k in KERNELS))


if __name__ == '__main__':
    main()
