"""Command-line tools of the package."""
