#!/usr/bin/env python3
"""Console entry point: tracktolearn_amd.runners.ttl_recognize_bundles.main
(the bundle of every streamline from an atlas of model lines)."""
from tracktolearn_amd.runners.ttl_recognize_bundles import main

if __name__ == '__main__':
    main()
