#!/usr/bin/env python
"""Per-launch values of the counters of one `rocprofv3 --pmc` pass for the solve kernel: python tools/pmc_per_launch.py DIR
(DIR: the pass's output directory, `-d`; CSV output).  One line per counter: the launches in dispatch order.  Developer tool."""
import csv
import glob
import os
import sys


def main():
    files = sorted(glob.glob(os.path.join(sys.argv[1], '**', '*counter_collection.csv'), recursive=True), key=os.path.getmtime)
    if not files:
        print('no counter_collection.csv under', sys.argv[1])
        return 1
    per = {}
    for row in csv.DictReader(open(files[-1])):
        if 'ipm_solve_kernel' in row['Kernel_Name']:
            per.setdefault(row['Counter_Name'], {}).setdefault(int(row['Dispatch_Id']), 0.0)
            per[row['Counter_Name']][int(row['Dispatch_Id'])] += float(row['Counter_Value'])
    for name in sorted(per):
        vals = [per[name][k] for k in sorted(per[name])]
        print('%-20s %d launches: %s' % (name, len(vals), ' '.join('%.6g' % v for v in vals)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
