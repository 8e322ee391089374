#!/usr/bin/env python3
"""Console entry point: tracktolearn_amd.runners.ttl_density.main
(the track density maps of a .trk / .tck on a reference grid)."""
from tracktolearn_amd.runners.ttl_density import main

if __name__ == '__main__':
    main()
