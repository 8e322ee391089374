#!/usr/bin/env python3
"""Console entry point: tracktolearn_amd.runners.ttl_bundle_profile.main
(the tract profiles of segmented bundles on a reference grid)."""
from tracktolearn_amd.runners.ttl_bundle_profile import main

if __name__ == '__main__':
    main()
